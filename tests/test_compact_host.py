"""CPU tests of the compact frame ring's model (tests/compact_ref.py): slots, k and the look-back rebuild the full
ring's stacks (frames_ref.StackModel) for every live row, with the one documented exception of a reset row's s' channel 3."""
import numpy as np
import pytest

import compact_ref as cr
import frames_ref as fr


def drive(n, capacity, steps, seed, max_batch=None, p_plain_done=0.0):
    """random episode lengths 1..5 per env (length 1: resets at consecutive steps), each episode end a done with a reset image;
    with probability p_plain_done a done without a reset. After every step every live row is checked."""
    rng = np.random.default_rng(seed)
    img = lambda m: rng.integers(0, 256, (m, 84, 84), dtype=np.uint8)          # gray 84 x 84: preprocess is the identity
    x0 = img(n)
    comp, full = cr.CompactRing(x0, capacity, max_batch or n), cr.FullRing(x0, capacity)
    left = rng.integers(1, 6, n)
    reset_rows, checked = 0, 0
    next_first = {}                                                              # row -> the first frame of its env's next episode
    for t in range(steps):
        x = img(n)
        left -= 1
        ends = left == 0
        plain = (rng.random(n) < p_plain_done) & ~ends
        dones = (ends | plain).astype(np.float32)
        slot = np.full(n, -1, np.int32)
        slot[ends] = np.arange(int(ends.sum()), dtype=np.int32)
        rx = img(int(ends.sum()))
        left[ends] = rng.integers(1, 6, int(ends.sum()))
        a, r = rng.integers(0, 3, n).astype(np.int32), rng.standard_normal(n).astype(np.float32)
        p1 = comp.observe(x, a, r, dones, slot, rx)
        p2 = full.observe(x, slot, rx)
        assert p1 == p2
        for e in range(n):                                                       # the rows just filed (overwritten ones included)
            next_first.pop(p1 + e, None)
            if ends[e]:
                next_first[p1 + e] = rx[slot[e]]
        live = np.arange(min(comp.ctr, capacity))
        s, s2 = comp.stacks(live)
        assert np.array_equal(s, full.s[live]), t                                # s of every row
        assert np.array_equal(s2 & np.uint32(0xffffff), full.s2[live] & np.uint32(0xffffff)), t      # s' channels 0..2
        was_reset = np.array([p in next_first for p in live])
        assert np.all(comp.d[live][was_reset] == 1)
        keep = ~was_reset
        assert np.array_equal(s2[keep], full.s2[live][keep]), t                  # s' of rows without a reset (d = 0 among them)
        for p in live[was_reset]:
            assert np.array_equal((s2[p] >> np.uint32(24)).astype(np.uint8), next_first[p]), (t, p)
            reset_rows += 1
        checked += len(live)
    return reset_rows, checked


@pytest.mark.parametrize("n,capacity,steps,seed", [(4, 4 * 40, 40, 1), (3, 3 * 5, 37, 2), (1, 6, 50, 3), (8, 8 * 3, 20, 4)])
def test_compact_model_matches_full_ring(n, capacity, steps, seed):
    """random episode lengths with length-1 episodes; the small capacities wrap the ring several times"""
    reset_rows, checked = drive(n, capacity, steps, seed)
    assert reset_rows > 0 and checked > 0


def test_compact_model_slack_and_plain_dones():
    """max_batch above n (more slack slots than needed) and dones without a reset image, which keep the stack going in both rings"""
    reset_rows, _ = drive(5, 5 * 4, 31, 7, max_batch=13, p_plain_done=0.2)
    assert reset_rows > 0


def test_compact_model_first_rows_and_gather():
    """the first rows repeat x_0 (k = 0), the n-step gather takes s' from the window's last row, and idx is clamped"""
    rng = np.random.default_rng(5)
    n, cap = 2, 8
    x0 = rng.integers(0, 256, (n, 84, 84), dtype=np.uint8)
    comp = cr.CompactRing(x0, cap, n)
    xs = [rng.integers(0, 256, (n, 84, 84), dtype=np.uint8) for _ in range(3)]
    for x in xs:
        comp.observe(x, np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32))
    s, s2 = comp.gather_frames(np.array([0, 1, -5, 99]), n_step=1)
    assert np.array_equal(s[0], fr.stack_bytes(fr.stack_of(x0[:1]))[0])
    assert np.array_equal(s2[0][..., 3], xs[0][0]) and np.array_equal(s2[0][..., :3], s[0][..., 1:])
    assert np.array_equal(s[2], s[0]) and np.array_equal(s[3], comp.gather_frames(np.array([cap - 1]))[0][0])
    s, s2 = comp.gather_frames(np.array([0]), n_step=3, n_envs=n)                # window rows 0, 2, 4: s' of row 4
    assert np.array_equal(s2[0][..., 3], xs[2][0]) and np.array_equal(s2[0][..., 2], xs[1][0]) and np.array_equal(s2[0][..., 1], xs[0][0])
    assert np.array_equal(s2[0][..., 0], x0[0])


def test_compact_bytes_per_row():
    """the layout's cost: one 7056-byte frame and four 4-byte scalars per row, against two 28 224-byte stacks"""
    compact, full = 84 * 84 + 4 * 4, 2 * 84 * 84 * 4 + 3 * 4
    assert compact <= 7100 and full / compact > 7.9
    assert (1 << 20) * compact < 7.5e9 < (1 << 20) * full / 7
