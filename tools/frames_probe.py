#!/usr/bin/env python3
"""Pixel envs on the device (dqn_cnn_env_observe, dqn_cnn_frames.h), measured:

  python tools/frames_probe.py --mode observe [--n 512 --F 2 --C 3 --H 210 --W 160 --reps 50 --rotate 1]
      the observe kernel alone, raw frames already on the device: device-event time per call, the algorithmic bytes
      n F H W C (raw) + 4 n 28 224 (one stack read; s, s' and the next stack written) + 12 n, and bytes / time as a share of the
      6.29 TB/s copy rate. --rotate K cycles through K raw buffers (K n F H W C bytes: K = 3 at the default shape is 310 MB, more
      than the 256 MB Infinity Cache). Run it under rocprofv3 --kernel-trace --stats for the kernel's own time.
  python tools/frames_probe.py --mode loop [--n 512 --steps 30]
      CnnVectorAgent(env=Catch(n)).env_step() end to end, and its parts timed one by one: act (CNN + epsilon-greedy + the actions to
      the host), the host env, staging + host-to-device copy, the observe call (kernel + launch + synchronise).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deep_q_learning_amd as dq  # noqa: E402
from deep_q_learning_amd.General.QLearning.cnn_agent import CnnVectorAgent  # noqa: E402
from deep_q_learning_amd.General.QLearning.frame_envs import Catch  # noqa: E402

COPY_RATE = 6.29e12          # MI355X_MICROARCH.md, HBM: measured float4 copy


def algorithmic_bytes(n, F, H, W, C, m=0):
    return (n + m) * F * H * W * C + 4 * n * 84 * 84 * 4 + 12 * n


def observe(a):
    n, F, H, W, C = a.n, a.F, a.H, a.W, a.C
    e = dq.CnnEngine(num_actions=6, max_batch=n, precision="bf16")
    e.replay_init(n * 8)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    raws = [torch.randint(0, 256, (n, F, H, W, C), dtype=torch.uint8, device="cuda", generator=g) for _ in range(a.rotate)]
    act = torch.zeros(n, dtype=torch.int32, device="cuda"); r = torch.zeros(n, device="cuda"); d = torch.zeros(n, device="cuda")
    e.env_reset_frames(raws[0])
    for k in range(5):
        e.env_observe(raws[k % a.rotate], act, r, d)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for k in range(a.reps):
        e.env_observe(raws[k % a.rotate], act, r, d)
    e1.record(); e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.reps
    b = algorithmic_bytes(n, F, H, W, C)
    e.close()
    return {"mode": "observe", "n": n, "F": F, "H": H, "W": W, "C": C, "rotate": a.rotate, "raw_MB_cycled": round(a.rotate * n * F * H * W * C / 1e6, 1),
            "us_per_call": round(us, 2), "algorithmic_MB": round(b / 1e6, 2), "TBps": round(b / us / 1e6, 3),
            "share_of_copy_rate": round(b / us / 1e6 / (COPY_RATE / 1e12), 3)}


def loop(a):
    n, S = a.n, a.steps
    env = Catch(n, seed=0)
    ag = CnnVectorAgent(num_actions=3, capacity=n * 8, batch_size=min(n, 512), env=env)
    for _ in range(3):
        ag.env_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(S):
        ag.env_step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / S
    # the parts, one at a time (each ends in a synchronise)
    parts = {"act_ms": 0.0, "env_ms": 0.0, "stage_copy_ms": 0.0, "observe_call_ms": 0.0}
    cnn = ag.cnn
    for _ in range(S):
        t = time.perf_counter()
        av = cnn.env_act(0.1); ah = av.cpu().numpy()
        parts["act_ms"] += time.perf_counter() - t; t = time.perf_counter()
        frames, rewards, dones, rf = env.step(ah)
        parts["env_ms"] += time.perf_counter() - t; t = time.perf_counter()
        slot = np.full(n, -1, np.int32); slot[dones] = np.arange(int(dones.sum()))
        up = cnn._upload([(frames, torch.uint8, frames.shape), (rewards, torch.float32, (n,)), (dones, torch.float32, (n,)),
                          (slot, torch.int32, (n,))] + ([(rf, torch.uint8, rf.shape)] if len(rf) else []))
        torch.cuda.synchronize()
        parts["stage_copy_ms"] += time.perf_counter() - t; t = time.perf_counter()
        cnn.env_observe(up[0], av, up[1], up[2], up[3], up[4] if len(rf) else None)
        torch.cuda.synchronize()
        parts["observe_call_ms"] += time.perf_counter() - t
    ag.close()
    out = {"mode": "loop", "n": n, "env_step_ms": round(step_ms, 3), "env_steps_per_s": round(1e3 / step_ms, 1),
           "transitions_per_s": round(n * 1e3 / step_ms)}
    out.update({k: round(v * 1e3 / S, 3) for k, v in parts.items()})
    out["raw_MB_per_step"] = round(n * 2 * 210 * 160 * 3 / 1e6, 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="observe", choices=["observe", "loop"])
    ap.add_argument("--n", type=int, default=512); ap.add_argument("--F", type=int, default=2); ap.add_argument("--C", type=int, default=3)
    ap.add_argument("--H", type=int, default=210); ap.add_argument("--W", type=int, default=160)
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--rotate", type=int, default=1); ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_probe needs the GPU")
    print(json.dumps(observe(a) if a.mode == "observe" else loop(a)))
