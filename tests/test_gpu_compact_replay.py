"""GPU tests of the compact frame ring (dqn_cnn_replay_init_compact, dqn_cnn_compact.h): side by side with the
full ring on the same Catch observe calls -- gathers per the contract and against tests/compact_ref.py, bit-identical updates, the
agent end to end --, the refused calls, and the size of a 2^20-row ring."""
import ctypes as C

import numpy as np
import pytest

import compact_ref as cr
from _oracle import onp

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def dq(torch_cuda):
    import deep_q_learning_amd as pkg
    return pkg


def catch(**kw):
    from deep_q_learning_amd.General.QLearning.frame_envs import Catch
    return Catch(**kw)


def slots_of(dones):
    slot = np.full(len(dones), -1, np.int32)
    slot[dones] = np.arange(int(dones.sum()), dtype=np.int32)
    return slot


class Pair:
    """a full-ring and a compact-ring CnnEngine with the same parameters, fed the same Catch observe calls (random actions)"""

    def __init__(self, dq, n, cap, precision="f32", max_batch=None, seed=0, td_rule="reference"):
        self.n, self.cap = n, cap
        self.env = catch(n_envs=n, seed=seed)
        self.rng = np.random.default_rng(seed + 100)
        P = onp.cnn_init_params(3, seed)
        P = (P + 0.01 * self.rng.standard_normal(P.size)).astype(np.float32)
        P2 = (P + 0.01 * self.rng.standard_normal(P.size)).astype(np.float32)
        self.e = []
        for compact in (False, True):
            e = dq.CnnEngine(num_actions=3, max_batch=max_batch or n, precision=precision)
            e.set_params(P); e.set_params(P2, target=True); e.set_optimizer(lr=1e-3); e.set_td_rule(td_rule)
            e.replay_init(cap, compact=compact)
            self.e.append(e)
        x0 = self.env.reset()
        for e in self.e:
            e.env_reset_frames(x0, seed=1)
        self.ref = cr.CompactRing(x0, cap, max_batch or n)
        self.steps = 0

    def step(self):
        a = self.rng.integers(0, 3, self.n).astype(np.int32)
        frames, rewards, dones, reset_frames = self.env.step(a)
        slot = slots_of(dones)
        firsts = [e.env_observe(frames, a, rewards, dones, slot, reset_frames) for e in self.e]
        pos = self.ref.observe(frames, a, rewards, dones.astype(np.float32), slot, reset_frames)
        assert firsts == [pos, pos]
        self.steps += 1
        return dones

    def valid_rows(self, n_step):
        """ring positions of the rows whose n-step window is in the ring (counters [ctr - cap, ctr - (n_step - 1) n))"""
        ctr = self.steps * self.n
        c = np.arange(max(0, ctr - self.cap), ctr - (n_step - 1) * self.n)
        return (c % self.cap).astype(np.int32)

    def close(self):
        for e in self.e:
            e.close()


def check_gathers(p, n_step, idx=None):
    idx = p.valid_rows(n_step) if idx is None else idx
    if len(idx) == 0:
        return 0
    full, comp = ([host(t) for t in e.replay_gather(idx, n_step=n_step, n_envs=p.n, gamma=0.9)] for e in p.e)
    s_f, a_f, r_f, s2_f, d_f = full
    s_c, a_c, r_c, s2_c, d_c = comp
    assert np.array_equal(s_c, s_f) and np.array_equal(a_c, a_f) and np.array_equal(r_c, r_f) and np.array_equal(d_c, d_f)
    assert np.array_equal(s2_c[..., :3], s2_f[..., :3])
    row = np.clip(idx.astype(np.int64), 0, p.cap - 1)
    last = (row + (n_step - 1) * p.n) % p.cap
    kept = p.ref.d[last] == 0                                       # rows whose env went on (no reset on Catch without a done)
    assert np.array_equal(s2_c[kept], s2_f[kept])
    assert np.all(d_c[~kept] == 1)
    s_r, s2_r = p.ref.gather_frames(idx, n_step=n_step, n_envs=p.n)
    assert np.array_equal(s_c, s_r) and np.array_equal(s2_c, s2_r)
    return int((~kept).sum())


def test_compact_gather_matches_full_ring(dq):
    """16 Catch envs, a ring of 10 vector steps, 26 steps (it wraps twice): after every step the gathers of every valid row, 1- and
    3-step, match the full ring's per the contract and compact_ref bit for bit; out-of-range indices are clamped alike"""
    p = Pair(dq, 16, 16 * 10)
    terminal = 0
    for t in range(26):
        p.step()
        assert p.e[0].replay_size() == p.e[1].replay_size()
        for n_step in (1, 3):
            terminal += check_gathers(p, n_step)
    check_gathers(p, 3, np.array([-3, 0, p.cap - 1, p.cap + 5, 2 ** 31 - 1], np.int32))
    assert terminal > 0                                             # the exception was exercised
    p.close()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("td_rule", ["reference", "standard"])
def test_compact_update_bit_identical(dq, precision, n_step, td_rule):
    """update_replay on the compact ring = on the full ring, bit for bit: loss, |delta| and the parameters after each of 5 updates
    with the same idx / isw / gamma, on sampled rows that include terminal ones"""
    import torch
    B = 48
    p = Pair(dq, 16, 16 * 8, precision=precision, max_batch=B, seed=3, td_rule=td_rule)
    for _ in range(12):
        p.step()
    rng = np.random.default_rng(11)
    valid = p.valid_rows(n_step)
    terminal = 0
    for u in range(5):
        idx = rng.choice(valid, B, replace=False).astype(np.int32)
        isw = rng.uniform(0.2, 1.0, B).astype(np.float32)
        out = []
        for e in p.e:
            td = torch.empty(B, dtype=torch.float32, device=e.device)
            loss = e.update_from_replay(idx, isw, gamma=0.97, td_abs_out=td, want_loss=True, n_step=n_step, n_envs=p.n)
            out.append((loss, host(td), host(e.get_buffer("params"))))
        assert out[0][0] == out[1][0], (u, out[0][0], out[1][0])
        assert np.array_equal(out[0][1], out[1][1]), u
        assert np.array_equal(out[0][2], out[1][2]), u
        terminal += int(host(p.e[1].replay_gather(idx, n_step=n_step, n_envs=p.n)[4]).sum())
        p.step()                                                    # (the rings move between updates as in training)
        valid = p.valid_rows(n_step)
    assert terminal > 0
    p.close()


def test_compact_agent_bit_identical(dq):
    """CnnVectorAgent(env=Catch, n_step=3, compact_replay=True) against the default ring with the same seeds, 50 updates: the same
    losses and final parameters bit for bit (so the same actions throughout), no index errors"""
    from deep_q_learning_amd.General.QLearning.cnn_agent import CnnVectorAgent
    n, cap = 16, 16 * 32
    runs = []
    for compact in (False, True):
        ag = CnnVectorAgent(num_actions=3, capacity=cap, batch_size=32, precision="bf16", train_frequency=1, replace_frequency=20, lr=1e-4,
                            seed=4, n_step=3, env=catch(n_envs=n, seed=21), td_rule="standard", compact_replay=compact)
        ag.init_params(onp.cnn_init_params(3, 8))
        losses = ag.training(50, want_loss=True)
        runs.append((losses, host(ag.cnn.get_buffer("params")), ag.cnn.replay_size(), ag.index.device_errors()))
        ag.close()
    (l0, p0, z0, e0), (l1, p1, z1, e1) = runs
    assert len(l1) == 50 and all(np.isfinite(l1))
    assert l0 == l1 and np.array_equal(p0, p1) and z0 == z1
    assert z1[1] > cap                                              # the ring wrapped
    assert e0 == 0 and e1 == 0


def test_compact_mode_errors(dq):
    """replay_add, the synthetic env, a second env_reset_frames once rows exist and compact_replay without an env are refused"""
    import torch
    from deep_q_learning_amd.General.QLearning.cnn_agent import CnnVectorAgent
    n = 4
    e = dq.CnnEngine(num_actions=3, max_batch=8, precision="f32")
    lib, h, st = e.lib, e.h, e._s()
    assert e.replay_bytes() == 0
    e.replay_init(4 * n, compact=True)
    assert lib.dqn_cnn_replay_init(h, 4 * n) != 0 and lib.dqn_cnn_replay_init_compact(h, 4 * n) != 0     # the ring exists once
    s = torch.zeros((n, 84, 84, 4), dtype=torch.uint8, device=e.device)
    with pytest.raises(Exception, match="compact"):
        e.replay_add(s, np.zeros(n, np.int32), np.zeros(n, np.float32), s, np.zeros(n, np.float32))
    with pytest.raises(Exception, match="compact"):
        e.env_reset_synth(n)
    first = C.c_int64(0)
    assert lib.dqn_cnn_env_step_synth(h, 0.0, 0.0, C.byref(first), st) != 0 and "compact" in lib.dqn_last_error().decode()
    x = np.random.default_rng(0).integers(0, 256, (n, 2, 100, 100, 3), dtype=np.uint8)
    e.env_reset_frames(x)
    e.env_reset_frames(x)                                           # (again before the first row: allowed)
    e.env_observe(x, np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, bool))
    with pytest.raises(Exception, match="compact"):
        e.env_reset_frames(x)
    assert e.replay_size() == (n, n)
    e.close()
    with pytest.raises(ValueError, match="compact_replay"):
        CnnVectorAgent(num_actions=3, n_envs=8, capacity=64, batch_size=8, compact_replay=True)


def test_compact_ring_size(dq):
    """a 2^20-row compact ring (the Nature-DQN replay; the full ring would take 59 GB) fits in about 7.4 GB plus slack and staging,
    takes observe steps of Catch(512) and an update; the full ring's bytes are checked at a small capacity"""
    mb, cap = 512, 1 << 20
    small = dq.CnnEngine(num_actions=3, max_batch=mb, precision="bf16")
    small.replay_init(1024)
    assert small.replay_bytes() >= 1024 * (2 * 84 * 84 * 4 + 12) + 2 * mb * 84 * 84 * 4
    small.close()
    e = dq.CnnEngine(num_actions=3, max_batch=mb, precision="bf16")
    e.set_params(onp.cnn_init_params(3, 1)); e.set_params(onp.cnn_init_params(3, 1), target=True); e.set_optimizer(lr=1e-4)
    e.replay_init(cap, compact=True)
    got = e.replay_bytes()
    assert cap * 7056 < got <= cap * 7100 + 4 * mb * 7056 + 2 * mb * 28224 + (1 << 20), got
    env = catch(n_envs=mb, seed=5)
    e.env_reset_frames(env.reset())
    rng = np.random.default_rng(2)
    for _ in range(4):
        a = e.env_act(1.0)
        frames, r, d, rf = env.step(host(a))
        e.env_observe(frames, a, r, d, slots_of(d), rf)
    assert e.replay_size() == (4 * mb, 4 * mb)
    idx = rng.integers(0, 4 * mb, mb).astype(np.int32)
    loss = e.update_from_replay(idx, np.ones(mb, np.float32), gamma=0.99, want_loss=True)
    assert np.isfinite(loss)
    e.close()
