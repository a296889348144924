"""numpy restatement of the compact frame ring (dqn_cnn_compact.h): each preprocessed frame once in a plane of
capacity + 4 max_batch slots, per row its slot and k (its step within the episode, clamped to 3), the stacks put together at sample
time. FullRing is the full ring's rows (s, s' as whole stacks) fed the same observe calls, through frames_ref.StackModel."""
import numpy as np

import frames_ref as fr


class CompactRing:
    def __init__(self, first_images, capacity, max_batch):
        x0 = fr.preprocess(first_images)
        self.n, self.cap, self.cf = len(x0), int(capacity), int(capacity) + 4 * int(max_batch)
        assert self.cap % self.n == 0 and self.n <= max_batch
        self.plane = np.zeros((self.cf, 84, 84), np.uint8)
        self.slot = np.zeros(self.cap, np.int64)
        self.k = np.zeros(self.cap, np.int64)
        self.a = np.zeros(self.cap, np.int32)
        self.r = np.zeros(self.cap, np.float32)
        self.d = np.zeros(self.cap, np.float32)
        self.k_env = np.zeros(self.n, np.int64)
        self.ctr = 0
        self.plane[np.arange(self.n) % self.cf] = x0

    def observe(self, images, actions, rewards, dones, reset_slot=None, reset_images=None):
        """files rows [pos, pos + n); returns pos"""
        n, e = self.n, np.arange(self.n)
        nxt = fr.preprocess(images)
        reset = np.zeros(n, bool)
        if reset_slot is not None and reset_images is not None and len(reset_images):
            rs = fr.preprocess(reset_images)
            for i, j in enumerate(np.asarray(reset_slot)):
                if 0 <= j < len(rs):
                    nxt[i], reset[i] = rs[j], True
        pos = self.ctr % self.cap
        rows = pos + e
        self.slot[rows], self.k[rows] = (self.ctr + e) % self.cf, self.k_env
        self.a[rows], self.r[rows], self.d[rows] = actions, rewards, dones
        self.plane[(self.ctr + n + e) % self.cf] = nxt
        self.k_env = np.where(reset, 0, np.minimum(self.k_env + 1, 3))
        self.ctr += n
        return pos

    def _f(self, slot):
        return self.plane[np.asarray(slot) % self.cf]

    def stacks(self, rows):
        """u32 stacks (s, s') [len(rows), 84, 84] of the rows, channel 3 the newest"""
        rows = np.asarray(rows, np.int64)
        sl, k, n = self.slot[rows], self.k[rows], self.n
        s = [self._f(sl - np.minimum(3 - c, k) * n) for c in range(4)]
        s2 = [self._f(sl - np.minimum(2 - c, k) * n) for c in range(3)] + [self._f(sl + n)]
        pack = lambda ch: sum(x.astype(np.uint32) << np.uint32(8 * c) for c, x in enumerate(ch))
        return pack(s), pack(s2)

    def gather_frames(self, idx, n_step=1, n_envs=0):
        """the u8 [B, 84, 84, 4] (s, s') of replay_gather: idx clamped to the ring, s' of the n-step window's last row"""
        row = np.clip(np.asarray(idx, np.int64), 0, self.cap - 1)
        last = (row + (n_step - 1) * n_envs) % self.cap
        return fr.stack_bytes(self.stacks(row)[0]), fr.stack_bytes(self.stacks(last)[1])


class FullRing:
    """the full ring's s / s' rows for the same observe calls"""

    def __init__(self, first_images, capacity):
        self.model = fr.StackModel(first_images)
        self.n, self.cap, self.ctr = len(self.model.cur), int(capacity), 0
        self.s = np.zeros((self.cap, 84, 84), np.uint32)
        self.s2 = np.zeros((self.cap, 84, 84), np.uint32)

    def observe(self, images, reset_slot=None, reset_images=None):
        s, s2 = self.model.observe(images, reset_slot, reset_images)
        pos = self.ctr % self.cap
        self.s[pos:pos + self.n], self.s2[pos:pos + self.n] = s, s2
        self.ctr += self.n
        return pos
