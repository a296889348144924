"""CPU tests of the pixel-env feature: the numpy restatement of the preprocessing against an independent float64 area mean, its
fixed points, the Catch env (determinism, flicker, reset frames) and the protocol checks of frame_envs.reset_slots."""
import numpy as np
import pytest

import frames_ref as fr


def catch(**kw):
    from deep_q_learning_amd.General.QLearning.frame_envs import Catch
    return Catch(**kw)


def f64_area_mean(M):
    """the area mean of M [H, W] over each of the 84 x 84 output cells, from the overlap fractions in source pixels (float64)"""
    H, W = M.shape

    def frac(n):
        lo, hi = np.arange(84) * n / 84.0, (np.arange(84) + 1) * n / 84.0
        r = np.arange(n)
        return np.clip(np.minimum(r[None, :] + 1.0, hi[:, None]) - np.maximum(r[None, :] * 1.0, lo[:, None]), 0.0, None)

    fy, fx = frac(H), frac(W)
    return fy @ M.astype(np.float64) @ fx.T / ((H / 84.0) * (W / 84.0))


@pytest.mark.parametrize("H,W", [(210, 160), (250, 160), (84, 84), (97, 131), (512, 512), (85, 511)])
def test_restatement_matches_float_area_mean(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    for kind in ("random", "blocks"):
        if kind == "random":
            M = rng.integers(0, 256, (H, W))
        else:                                                       # large flat regions: many exact-half ties
            M = np.kron(rng.integers(0, 2, (H // 7 + 1, W // 7 + 1)) * 255, np.ones((7, 7), np.int64))[:H, :W]
        x = M.astype(np.uint8)[None, None, :, :, None]
        got = fr.preprocess(x)[0].astype(np.int64)
        mean = f64_area_mean(M)
        S = fr.area_sums(M[None])[0]
        tie = (2 * S) % (2 * H * W) == H * W                        # exact half: decided in integers
        assert np.all(np.abs(got - mean) <= 0.5 + 1e-9)
        assert np.array_equal(got[~tie], np.floor(mean[~tie] + 0.5).astype(np.int64))
        assert np.array_equal(got[tie], np.floor(mean[tie]).astype(np.int64) + 1)     # half up


def test_exact_half_rounds_up():
    """168 x 168 -> 84 x 84 is a 2 x 2 mean: columns alternating v, v + 1 make every mean v + 1/2, which rounds to v + 1"""
    for v in (0, 100, 254):
        M = np.tile(np.array([v, v + 1], np.uint8), (168, 84))
        assert np.all(np.abs(f64_area_mean(M.astype(np.int64)) - (v + 0.5)) < 1e-9)
        assert np.all(fr.preprocess(M[None, None, :, :, None]) == v + 1)


def test_constant_image_and_identity():
    rng = np.random.default_rng(3)
    for v in (0, 1, 128, 254, 255):
        for H, W in ((210, 160), (97, 131), (512, 84)):
            x = np.full((1, 2, H, W, 1), v, np.uint8)
            assert np.all(fr.preprocess(x) == v)
    x = rng.integers(0, 256, (3, 1, 84, 84, 3), dtype=np.uint8)
    assert np.array_equal(fr.preprocess(x), fr.luma(x[:, 0]).astype(np.uint8))            # 84 x 84: identity on luma
    rgb = np.array([[[[[255, 255, 255]]]]], np.uint8)
    assert fr.luma(rgb)[0, 0, 0, 0] == 255                                                # the weights sum to 2^14


def test_luma_and_max_order():
    """gray first, then the max over F (not the max per colour channel)"""
    a = np.zeros((1, 2, 84, 84, 3), np.uint8)
    a[0, 0, ..., 0] = 200                       # red: Y = 60
    a[0, 1, ..., 1] = 100                       # green: Y = 59
    out = fr.preprocess(a)
    assert np.all(out == (4899 * 200 + 8192) >> 14)


def test_stack_helpers():
    rng = np.random.default_rng(5)
    s = rng.integers(0, 2 ** 32, (2, 84, 84), dtype=np.uint64).astype(np.uint32)
    out = rng.integers(0, 256, (2, 84, 84), dtype=np.uint8)
    b, b2 = fr.stack_bytes(s), fr.stack_bytes(fr.push(s, out))
    assert np.array_equal(b2[..., :3], b[..., 1:]) and np.array_equal(b2[..., 3], out)
    assert np.all(fr.stack_bytes(fr.stack_of(out)) == out[..., None])
    assert np.array_equal(fr.u32_of(b), s)


def test_catch_deterministic_and_flicker():
    e1, e2, e3 = catch(n_envs=7, seed=4), catch(n_envs=7, seed=4), catch(n_envs=7, seed=5)
    f1, f2, f3 = e1.reset(), e2.reset(), e3.reset()
    assert f1.shape == (7, 2, 210, 160, 3) and f1.dtype == np.uint8
    assert np.array_equal(f1, f2) and not np.array_equal(f1, f3)
    rng = np.random.default_rng(0)
    ball = np.array(e1.ball_c)
    saw_done = False
    for t in range(30):
        a = rng.integers(0, 3, 7).astype(np.int32)
        o1, o2 = e1.step(a), e2.step(a)
        for u, v in zip(o1, o2):
            assert np.array_equal(u, v)
        frames, rewards, dones, reset_frames = o1
        assert rewards.dtype == np.float32 and dones.dtype == bool and reset_frames.shape == (int(dones.sum()), 2, 210, 160, 3)
        has_ball = np.all(frames == ball, axis=-1).reshape(7, 2, -1).any(axis=-1)
        assert np.array_equal(has_ball.sum(axis=1), np.ones(7))                    # exactly one raw frame shows the ball
        assert np.all(has_ball[:, (t % 9 + 1) % 2])                               # alternating by episode step
        assert np.all(np.abs(rewards[dones]) == 1) and np.all(rewards[~dones] == 0)
        if dones.any():
            saw_done = True
            assert (t + 1) % 9 == 0
            top = reset_frames[:, 0, 20:39]                                       # a new episode: the ball in the top row, frame 0
            assert np.all(np.all(top == ball, axis=-1).any(axis=(1, 2)))
            assert not np.all(reset_frames[:, 1] == ball, axis=-1).any()
    assert saw_done


def test_catch_gray_is_the_luma_of_rgb():
    rgb, gray = catch(n_envs=3, seed=9), catch(n_envs=3, seed=9, frames=1, channels=1)
    a, b = rgb.reset(), gray.reset()
    assert b.shape == (3, 1, 210, 160, 1)
    assert np.array_equal(fr.preprocess(a), fr.preprocess(b)) and np.array_equal(fr.luma(a[:, 0]), b[:, 0, ..., 0])
    for t in range(5):
        act = np.array([0, 1, 2], np.int32)
        fa, ra, da, _ = rgb.step(act)
        fb, rb, db, _ = gray.step(act)
        assert np.array_equal(ra, rb) and np.array_equal(da, db)
        assert np.array_equal(fr.preprocess(fa), fr.preprocess(fb))                # same state: same preprocessed image
    colours = {tuple(v) for v in catch(n_envs=1).RGB.values()}
    lumas = {int(fr.luma(np.array(c, np.uint8)[None])[0]) for c in colours}
    assert len(lumas) == 3 and 0 not in lumas                                      # distinct greys, non-black background


def test_reset_slots_checks():
    from deep_q_learning_amd.General.QLearning.frame_envs import reset_slots
    d = np.array([0, 1, 0, 1, 1], bool)
    assert reset_slots(d, np.zeros((3, 2, 84, 84, 3), np.uint8), 5).tolist() == [-1, 0, -1, 1, 2]
    assert reset_slots(np.zeros(5, bool), np.zeros((0, 84, 84), np.uint8), 5).tolist() == [-1] * 5
    with pytest.raises(ValueError):
        reset_slots(d, np.zeros((2, 84, 84), np.uint8), 5)
    with pytest.raises(ValueError):
        reset_slots(d[:4], np.zeros((3, 84, 84), np.uint8), 5)


def test_image_geometry():
    from deep_q_learning_amd.cnn import image_geometry
    assert image_geometry((8, 2, 210, 160, 3)) == (8, 2, 210, 160, 3)
    assert image_geometry((8, 210, 160, 3)) == (8, 1, 210, 160, 3)
    assert image_geometry((8, 2, 210, 160)) == (8, 2, 210, 160, 1)
    assert image_geometry((8, 210, 160)) == (8, 1, 210, 160, 1)
    for bad in ((8, 3, 210, 160, 3), (8, 2, 83, 160, 3), (8, 2, 210, 513, 1), (8, 2, 210, 160, 2), (8, 210)):
        with pytest.raises(ValueError):
            image_geometry(bad)
