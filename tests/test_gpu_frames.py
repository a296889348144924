"""GPU tests of the pixel envs (dqn_cnn_env_reset_frames / dqn_cnn_env_act / dqn_cnn_env_observe): the device preprocessing and
stacking bit for bit against tests/frames_ref.py, acting against dqn_cnn_act, the mode errors and the agent loop on Catch."""
import ctypes as C
import time

import numpy as np
import pytest

import frames_ref as fr
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


def images(kind, n, F, H, W, Cc, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (n, F, H, W, Cc), dtype=np.uint8)
    if kind == "white":
        return np.full((n, F, H, W, Cc), 255, np.uint8)
    env = catch(n_envs=n, seed=seed, frames=F, channels=Cc)
    env.reset()
    return env.step(np.arange(n, dtype=np.int32) % 3)[0]


GEOS = [(210, 160, 3, 2), (210, 160, 1, 1), (250, 160, 3, 2), (84, 84, 3, 1), (97, 131, 3, 2),
        (512, 512, 3, 2), (511, 509, 3, 2)]     # the largest image: 38 of the 40 LDS rows, five source rows per staging pass


@pytest.mark.parametrize("H,W,Cc,F", GEOS)
def test_frames_preprocess_bitexact(dq, H, W, Cc, F):
    """one reset + one observe: the ring's s = the reset image four times, s' channel 3 = the restatement of the step image bit for
    bit, s' channels 0..2 = s channels 1..3"""
    n = 5
    kinds = ["random", "white"] + (["catch"] if (H, W) == (210, 160) else [])
    for kind in kinds:
        e = dq.CnnEngine(num_actions=3, max_batch=8, precision="f32")
        e.replay_init(n)
        x0, x1 = images("random", n, F, H, W, Cc, 1), images(kind, n, F, H, W, Cc, 2)
        shape = (n, H, W, Cc) if F == 1 else (n, F, H, W) if Cc == 1 else (n, F, H, W, Cc)       # the optional axes left out
        e.env_reset_frames(x0.reshape(shape), seed=3)
        first = e.env_observe(x1.reshape(shape), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, bool))
        assert first == 0
        s, a, r, s2, d = (host(t) for t in e.replay_gather(np.arange(n, dtype=np.int32)))
        want = fr.preprocess(x1)
        assert np.array_equal(s2[..., 3], want), kind
        assert np.array_equal(s2[..., :3], s[..., 1:]), kind
        assert np.array_equal(s, fr.stack_bytes(fr.stack_of(fr.preprocess(x0)))), kind
        e.close()


def test_frames_stack_and_reset_bitexact(dq):
    """a scripted 9-step sequence with resets -- done on the first step, all done at once, none done, a done without a reset slot,
    out-of-range slots -- against the host restatement of every ring field s, a, r, d, s'"""
    n, H, W, Cc, F, steps = 4, 210, 160, 3, 2, 9
    rng = np.random.default_rng(17)
    e = dq.CnnEngine(num_actions=3, max_batch=8, precision="f32")
    e.replay_init(n * steps)
    x0 = rng.integers(0, 256, (n, F, H, W, Cc), dtype=np.uint8)
    e.env_reset_frames(x0, seed=1)
    model = fr.StackModel(x0)
    script = [   # (dones, reset_slot, m)
        ([1, 0, 0, 0], [0, -1, -1, -1], 1),
        ([0, 0, 0, 0], [-1, -1, -1, -1], 0),
        ([1, 1, 1, 1], [0, 1, 2, 3], 4),
        ([0, 1, 0, 0], [-1, -1, -1, -1], 0),            # done, no reset slot
        ([0, 0, 1, 1], [-1, -1, 5, -7], 1),             # slots outside [0, m): no reset
        ([1, 0, 0, 1], [1, -1, -1, 0], 2),
        ([0, 0, 0, 0], [-1, -1, -1, -1], 0),
        ([0, 1, 0, 0], [-1, 0, -1, -1], 1),
        ([0, 0, 0, 0], None, 0),
    ]
    want = {k: [] for k in "s a r d s2".split()}
    for t, (dn, slot, m) in enumerate(script):
        x = rng.integers(0, 256, (n, F, H, W, Cc), dtype=np.uint8)
        rx = rng.integers(0, 256, (m, F, H, W, Cc), dtype=np.uint8)
        a = rng.integers(0, 3, n).astype(np.int32)
        r = rng.standard_normal(n).astype(np.float32)
        d = np.array(dn, bool)
        first = e.env_observe(x, a, r, d, None if slot is None else np.array(slot, np.int32), rx if m else None)
        assert first == t * n
        s, s2 = model.observe(x, slot, rx)
        for k, v in zip("s a r d s2".split(), (fr.stack_bytes(s), a, r, d.astype(np.float32), fr.stack_bytes(s2))):
            want[k].append(v)
    got = dict(zip("s a r s2 d".split(), (host(t) for t in e.replay_gather(np.arange(n * steps, dtype=np.int32)))))
    for k in want:
        assert np.array_equal(got[k], np.concatenate(want[k])), k
    e.close()


def test_frames_env_act_matches_cnn_act(dq):
    """env_act = dqn_cnn_act on the same stacks with (seed, env step), at epsilon 0 and 0.3"""
    n, seed = 24, 7
    rng = np.random.default_rng(2)
    e = dq.CnnEngine(num_actions=3, max_batch=32, precision="f32")
    P = onp.cnn_init_params(3, 5); P = (P + 0.01 * rng.standard_normal(P.size)).astype(np.float32)
    e.set_params(P)
    e.replay_init(n * 4)
    x0 = rng.integers(0, 256, (n, 2, 210, 160, 3), dtype=np.uint8)
    e.env_reset_frames(x0, seed=seed)
    cur = fr.stack_bytes(fr.stack_of(fr.preprocess(x0)))
    for step in range(3):
        for eps in (0.0, 0.3):
            got = host(e.env_act(eps))
            assert np.array_equal(got, host(e.act(cur, eps, seed, step))), (step, eps)
        if step == 0:
            assert len(set(host(e.env_act(0.3)))) > 1
        x = rng.integers(0, 256, (n, 2, 210, 160, 3), dtype=np.uint8)
        first = e.env_observe(x, np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, bool))
        cur = host(e.replay_gather(np.arange(first, first + n, dtype=np.int32))[3])
    e.close()


def test_frames_mode_errors(dq):
    """each misuse returns an error with a message and faults nothing: observe / act before a reset, a geometry outside the limits,
    the synthetic env after reset_frames and the pixel env after reset_synth, either env on a new ring"""
    import torch
    e = dq.CnnEngine(num_actions=3, max_batch=8, precision="f32")
    lib, h, st = e.lib, e.h, e._s()
    n = 4
    raw = torch.zeros((n, 2, 100, 100, 3), dtype=torch.uint8, device=e.device)
    a = torch.zeros(n, dtype=torch.int32, device=e.device); f = torch.zeros(n, dtype=torch.float32, device=e.device)
    first = C.c_int64(0)
    P = lambda t: C.c_void_p(t.data_ptr())

    def refused(rc):
        msg = lib.dqn_last_error().decode()
        return rc != 0 and len(msg) > 0

    observe = lambda: lib.dqn_cnn_env_observe(h, P(raw), P(a), P(f), P(f), None, None, 0, C.byref(first), st)
    act = lambda: lib.dqn_cnn_env_act(h, 0.0, P(a), st)
    synth = lambda: lib.dqn_cnn_env_step_synth(h, 0.0, 0.0, C.byref(first), st)
    reset = lambda F, H, W, Cc: lib.dqn_cnn_env_reset_frames(h, n, P(raw), F, H, W, Cc, 0, st)
    assert refused(observe()) and refused(act()) and refused(reset(2, 100, 100, 3))      # no ring, no envs
    e.replay_init(4 * n)
    assert refused(observe()) and refused(act()) and refused(synth())                    # a new ring: no env of either kind
    for geo in ((3, 100, 100, 3), (0, 100, 100, 3), (2, 83, 100, 3), (2, 100, 513, 1), (1, 100, 100, 2), (2, 600, 100, 1)):
        assert refused(reset(*geo)), geo
    assert refused(observe())                                                            # the refused resets started nothing
    assert lib.dqn_cnn_env_reset_frames(h, 3, P(raw), 2, 100, 100, 3, 0, st) != 0         # n must divide the capacity
    assert reset(2, 100, 100, 3) == 0
    assert refused(synth())                                                              # reset_frames ended the synthetic env
    assert act() == 0 and observe() == 0
    assert lib.dqn_cnn_env_reset_synth(h, n, 0, st) == 0
    assert refused(observe()) and refused(act())                                         # reset_synth ended the pixel env
    assert synth() == 0
    assert reset(2, 100, 100, 3) == 0 and refused(synth()) and observe() == 0
    assert refused(lib.dqn_cnn_replay_init(h, 4 * n)) and act() == 0 and observe() == 0          # a live ring is never replaced
    assert lib.dqn_cnn_env_reset_synth(h, n, 0, st) == 0
    assert refused(lib.dqn_cnn_replay_init(h, 4 * n)) and synth() == 0
    torch.cuda.synchronize()
    assert e.replay_size()[1] == 5 * n
    e.env_reset_frames(raw)
    with pytest.raises(ValueError):
        e.env_observe(np.zeros((n, 2, 100, 90, 3), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, bool))
    with pytest.raises(ValueError):                                                      # reset images need their slots
        e.env_observe(np.zeros((n, 2, 100, 100, 3), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.float32), np.ones(n, bool),
                      None, np.zeros((n, 2, 100, 100, 3), np.uint8))
    e.close()


class Recording:
    """a pixel env that records what passes through it"""

    def __init__(self, env):
        self.env, self.n_envs, self.log = env, env.n_envs, []

    def reset(self):
        self.first = self.env.reset()
        return self.first

    def step(self, actions):
        out = self.env.step(actions)
        self.log.append((np.array(actions), out))
        return out


def test_frames_agent_loop_catch(dq):
    """CnnVectorAgent(env=Catch, n_step=3), 50 updates: finite losses; every ring row equals the restatement applied to the frames
    the env produced; the stored actions are the ones env.step received"""
    from deep_q_learning_amd.General.QLearning.cnn_agent import CnnVectorAgent
    n, cap = 16, 16 * 128
    env = Recording(catch(n_envs=n, seed=21))
    ag = CnnVectorAgent(num_actions=3, capacity=cap, batch_size=32, precision="bf16", train_frequency=1, replace_frequency=20, lr=1e-4,
                        seed=4, n_step=3, env=env)
    ag.init_params(onp.cnn_init_params(3, 8))
    losses = ag.training(50, want_loss=True)
    assert len(losses) == 50 and all(np.isfinite(l) for l in losses)
    T = ag.env_steps
    assert T == len(env.log) and T * n <= cap and ag.cnn.replay_size() == (T * n, T * n)
    model = fr.StackModel(env.first)
    want_s, want_s2, want_a, want_r, want_d = [], [], [], [], []
    for acts, (frames, rewards, dones, reset_frames) in env.log:
        slot = np.full(n, -1, np.int32); slot[dones] = np.arange(int(dones.sum()))
        s, s2 = model.observe(frames, slot, reset_frames)
        want_s.append(fr.stack_bytes(s)); want_s2.append(fr.stack_bytes(s2))
        want_a.append(acts); want_r.append(rewards); want_d.append(dones.astype(np.float32))
    s, a, r, s2, d = (host(t) for t in ag.cnn.replay_gather(np.arange(T * n, dtype=np.int32)))
    assert np.array_equal(a, np.concatenate(want_a)) and np.array_equal(r, np.concatenate(want_r)) and np.array_equal(d, np.concatenate(want_d))
    assert np.array_equal(s, np.concatenate(want_s)) and np.array_equal(s2, np.concatenate(want_s2))
    assert d.sum() > 0 and ag.index.device_errors() == 0
    ag.close()


def test_cnn_td_rule_standard(dq):
    """dqn_cnn_set_td_rule(DQN_TD_STANDARD): the loss of one update is the loss of the targets q with q[a] replaced by
    r + (1 - d) gamma Q_target(s')[argmax Q(s')] (r at a terminal row); the default stays the reference's rule (q[a] + r there)"""
    A_, B, g = 3, 24, 0.9
    rng = np.random.default_rng(31)
    P = onp.cnn_init_params(A_, 3); P = (P + 0.01 * rng.standard_normal(P.size)).astype(np.float32)
    P2 = (P + 0.01 * rng.standard_normal(P.size)).astype(np.float32)
    s, s2 = (rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8) for _ in range(2))
    a = rng.integers(0, A_, B).astype(np.int32); r = rng.standard_normal(B).astype(np.float32)
    d = (np.arange(B) % 3 == 0).astype(np.float32)
    engines = []
    for rule in ("standard", "reference", None):
        e = dq.CnnEngine(num_actions=A_, max_batch=64, precision="f32")
        e.set_params(P); e.set_params(P2, target=True); e.set_optimizer(lr=1e-3)
        if rule:
            e.set_td_rule(rule)
        engines.append(e)
    q, nq, nt = host(engines[2].forward(s)), host(engines[2].forward(s2)), host(engines[2].forward(s2, target=True))
    T = q.copy()
    T[np.arange(B), a] = r + (np.float32(1) - d) * (np.float32(g) * nt[np.arange(B), nq.argmax(1)])
    assert np.array_equal(T[d == 1, a[d == 1]], r[d == 1])
    T_ref = q.copy()
    T_ref[np.arange(B), a] = q[np.arange(B), a] + r + (np.float32(1) - d) * (np.float32(g) * nt[np.arange(B), nq.argmax(1)] - q[np.arange(B), a])
    want, want_ref = engines[2].grads(s, T), engines[2].grads(s, T_ref)
    assert abs(want - want_ref) > 1e-5                                                  # (8 terminal rows of 24)
    got = engines[0].update(s, a, r, s2, d, gamma=g, want_loss=True)
    assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (got, want, want_ref)
    ref = dq.CnnEngine(num_actions=A_, max_batch=64, precision="f32")
    ref.set_params(P); ref.set_params(P2, target=True); ref.set_optimizer(lr=1e-3)
    ref.update(s, a, r, s2, d, gamma=g)
    got_ref = engines[1].update(s, a, r, s2, d, gamma=g, want_loss=True)              # rule "reference" == the default
    assert abs(got_ref - want_ref) <= 1e-6 * max(1.0, abs(want_ref)), (got_ref, want_ref)
    assert np.array_equal(host(engines[1].get_buffer("params")), host(ref.get_buffer("params")))
    assert not np.array_equal(host(engines[1].get_buffer("params")), host(engines[0].get_buffer("params")))
    for e in engines + [ref]:
        e.close()


def greedy_catch_rate(dq, params, precision, n=64, episodes=512, seed=1234):
    """the greedy (epsilon = 0) catch rate over >= episodes Catch episodes, on an engine of its own (env_act + env_observe)"""
    e = dq.CnnEngine(num_actions=3, max_batch=n, precision=precision)
    e.set_params(params); e.replay_init(n)
    env = catch(n_envs=n, seed=seed)
    e.env_reset_frames(env.reset())
    done = caught = 0
    while done < episodes:
        a = e.env_act(0.0)
        frames, r, d, rf = env.step(host(a))
        done += int(d.sum()); caught += int((r > 0).sum())
        slot = np.full(n, -1, np.int32); slot[d] = np.arange(int(d.sum()))
        e.env_observe(frames, a, r, d, slot, rf)
    e.close()
    return caught / done


def test_catch_learns(dq):
    """train on Catch, then play greedily: >= 0.9 of >= 512 episodes caught, against the untrained net's rate. Catch pays only at
    terminal steps, so this takes the standard TD rule (td_rule="standard"; the reference's terminal target q[a] + r diverges).
    Config: 32 envs, batch 128, lr 2.5e-4, gamma 0.9, 3-step returns, PER, target sync every 100 updates, one update per vector
    step; evaluated every 250 updates, stopping at the first evaluation that reaches 0.9 (at most 4 000 updates, 100 s)."""
    from deep_q_learning_amd.General.QLearning.cnn_agent import CnnVectorAgent
    t0 = time.time()
    ag = CnnVectorAgent(num_actions=3, capacity=32 * 256, batch_size=128, precision="bf16", gamma=0.9, epsilon=1.0,
                        epsilon_decay_rate=0.995, min_epsilon=0.05, train_frequency=1, replace_frequency=100, lr=2.5e-4, seed=0, n_step=3,
                        env=catch(n_envs=32, seed=0), td_rule="standard")
    P = onp.cnn_init_params(3, 0)
    ag.init_params(P)
    before = greedy_catch_rate(dq, P, "bf16")
    rate, updates = before, 0
    while updates < 4000 and time.time() - t0 < 100:
        losses = ag.training(250, want_loss=True)
        updates += 250
        assert np.all(np.isfinite(losses))
        rate = greedy_catch_rate(dq, host(ag.cnn.get_buffer("params")), "bf16")
        if rate >= 0.9:
            break
    took = time.time() - t0
    print(f"catch rate {before:.3f} -> {rate:.3f} after {updates} updates ({ag.env_steps} vector steps of 32 envs), {took:.1f} s")
    assert rate >= 0.9 and rate > before
    assert took < 120
    ag.close()


def test_agent_checks_the_env(dq):
    from deep_q_learning_amd.General.QLearning.cnn_agent import CnnVectorAgent
    with pytest.raises(ValueError):
        CnnVectorAgent(num_actions=6, capacity=64, batch_size=16, env=catch(n_envs=8))          # Catch has 3 actions
