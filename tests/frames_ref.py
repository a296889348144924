"""numpy restatement of the pixel-env preprocessing and frame stacking (dqn_cnn_frames.h, DESIGN.md "Pixel envs"): integer
arithmetic throughout, so the device must match it bit for bit."""
import numpy as np


def as_images(x):
    """[n, F, H, W, C] view of a batch of env images whose F / C axes may be left out when 1 (as CnnEngine.image_geometry)"""
    x = np.asarray(x)
    if x.ndim == 3:
        return x[:, None, :, :, None]
    if x.ndim == 4:
        return x[..., None] if x.shape[1] in (1, 2) else x[:, None]
    return x


def luma(x):
    """Y of u8 [..., C] (C = 3: OpenCV's integer weights, C = 1: the input) as int64 [...]"""
    x = x.astype(np.int64)
    if x.shape[-1] == 1:
        return x[..., 0]
    return (4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14


def area_weights(H):
    """wr[i][r] = overlap of output row i = [H i, H i + H) and source row r = [84 r, 84 r + 84), in 1/84 source pixels"""
    i = np.arange(84, dtype=np.int64)[:, None]
    r = np.arange(H, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum(84 * (r + 1), H * (i + 1)) - np.maximum(84 * r, H * i))


def area_sums(M):
    """S = sum_r sum_c wr wc M for M int [n, H, W] -> int64 [n, 84, 84]"""
    H, W = M.shape[1:]
    return np.einsum("ir,nrc,jc->nij", area_weights(H), M.astype(np.int64), area_weights(W), optimize=True)


def preprocess(x):
    """u8 [n, 84, 84]: luma, max over the F frames, exact area resize rounded half up"""
    x = as_images(x)
    M = luma(x).max(axis=1)
    H, W = M.shape[1:]
    S = area_sums(M)
    return ((2 * S + H * W) // (2 * H * W)).astype(np.uint8)


def stack_of(out):
    """u32 stacks [n, 84, 84] holding out in all four channels (gym FrameStack.reset)"""
    return out.astype(np.uint32) * np.uint32(0x01010101)


def push(stack, out):
    """the stack shifted by one frame with out appended as channel 3 (the newest)"""
    return (stack >> np.uint32(8)) | (out.astype(np.uint32) << np.uint32(24))


def stack_bytes(stack):
    """u32 stacks [n, 84, 84] -> the CNN's u8 [n, 84, 84, 4] (byte k = channel k)"""
    return np.ascontiguousarray(stack.astype("<u4")).view(np.uint8).reshape(stack.shape + (4,))


def u32_of(frames):
    """u8 [n, 84, 84, 4] -> u32 stacks [n, 84, 84]"""
    return np.ascontiguousarray(frames).view("<u4").reshape(frames.shape[:3]).astype(np.uint32)


class StackModel:
    """host restatement of the envs' stacks across observe calls: returns the ring rows (s, s2) of each step"""

    def __init__(self, first_images):
        self.cur = stack_of(preprocess(first_images))

    def observe(self, images, reset_slot=None, reset_images=None):
        s = self.cur.copy()
        s2 = push(s, preprocess(images))
        nxt = s2.copy()
        if reset_slot is not None and reset_images is not None and len(reset_images):
            rs = stack_of(preprocess(reset_images))
            for e, k in enumerate(np.asarray(reset_slot)):
                if 0 <= k < len(rs):
                    nxt[e] = rs[k]
        self.cur = nxt
        return s, s2
