#!/usr/bin/env python3
"""The compact frame ring (dqn_cnn_replay_init_compact, dqn_cnn_compact.h) against the full ring, measured:

  python tools/compact_probe.py --mode observe [--n 512 --reps 50]
      dqn_cnn_env_observe on a full and on a compact ring (random RGB 210 x 160 frame pairs on the device, a reset every 8 steps
      per env), alternated in blocks: device-event time per call.
  python tools/compact_probe.py --mode gather [--B 512,8192 --reps 50]
      dqn_cnn_replay_gather (1-step) from a full and a compact ring of 64 vector steps of 512 envs, into preallocated outputs,
      alternated: time per call, the bytes each kernel must move (compact: 5 frames of 7 056 bytes read and 2 stacks of 28 224
      written per sample; full: 2 stacks read and 2 written) and bytes / time as a share of the 6.29 TB/s copy rate.
  python tools/compact_probe.py --mode update [--B 512 --reps 50]
      dqn_cnn_update_replay in bf16 on the two rings, alternated in blocks of reps: ms per update and the ratio compact / full.
Device-event times include the launch; run under rocprofv3 --kernel-trace --stats for the kernels' own times. One JSON line per
mode."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deep_q_learning_amd as dq  # noqa: E402
from deep_q_learning_amd import _lib as L  # noqa: E402

COPY_RATE = 6.29e12          # MI355X_MICROARCH.md, HBM: measured float4 copy
STACK, FRAME = 84 * 84 * 4, 84 * 84


def rings(n, steps, max_batch, precision="bf16", compact_first=False):
    """[full, compact] engines fed the same `steps` observe calls of n random frame pairs (resets every 8 steps, staggered), the
    compact one created first when compact_first"""
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    raw = [torch.randint(0, 256, (n, 2, 210, 160, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2)]
    a = torch.zeros(n, dtype=torch.int32, device="cuda"); r = torch.zeros(n, device="cuda")
    es = []
    for compact in ((True, False) if compact_first else (False, True)):
        e = dq.CnnEngine(num_actions=6, max_batch=max_batch, precision=precision)
        e.replay_init(n * steps, compact=compact)
        e.set_optimizer(lr=1e-4)
        e.env_reset_frames(raw[0])
        es.append(e)
    env = torch.arange(n, device="cuda")
    for t in range(steps):
        dn = ((env + t) % 8 == 7)
        slot = torch.where(dn, torch.cumsum(dn.int(), 0) - 1, torch.full_like(env, -1)).int()
        m = int(dn.sum())
        for e in es:
            e.env_observe(raw[t % 2], a, r, dn.float(), slot, raw[1][:m] if m else None)
    torch.cuda.synchronize()
    return (es[::-1] if compact_first else es), raw, a, r


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternate(fns, reps, rounds=4):
    """[us per call] of each fn, blocks of reps alternated over rounds; the minimum block of each"""
    best = [float("inf")] * len(fns)
    for f in fns:
        timed(f, 3)
    for _ in range(rounds):
        for k, f in enumerate(fns):
            best[k] = min(best[k], timed(f, reps))
    return best


def observe(a):
    n = a.n
    es, raw, act, r = rings(n, 8, n)
    d = torch.zeros(n, device="cuda")
    fns = [lambda e=e: e.env_observe(raw[0], act, r, d) for e in es]
    full, comp = alternate(fns, a.reps)
    for e in es:
        e.close()
    return {"mode": "observe", "n": n, "F": 2, "H": 210, "W": 160, "C": 3, "full_us": round(full, 2), "compact_us": round(comp, 2),
            "ratio": round(comp / full, 3)}


def gather(a):
    out = {"mode": "gather"}
    n, steps = 512, 64
    Bs = [int(b) for b in a.B.split(",")]
    es, *_ = rings(n, steps, n)
    lib = es[0].lib
    for B in Bs:
        idx = torch.randint(0, n * steps, (B,), dtype=torch.int32, device="cuda")
        s = torch.empty((B, 84, 84, 4), dtype=torch.uint8, device="cuda"); s2 = torch.empty_like(s)
        ai = torch.empty(B, dtype=torch.int32, device="cuda"); rr = torch.empty(B, device="cuda"); dd = torch.empty(B, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())

        def call(e):
            L.check(lib.dqn_cnn_replay_gather(e.h, P(idx), B, 1, 0, 0.99, P(s), P(ai), P(rr), P(s2), P(dd), e._s()))
        full, comp = alternate([lambda e=e: call(e) for e in es], a.reps)
        bf, bc = B * (4 * STACK + 12), B * (5 * FRAME + 2 * STACK + 16)
        out[f"B{B}"] = {"full_us": round(full, 2), "compact_us": round(comp, 2), "full_MB": round(bf / 1e6, 1), "compact_MB": round(bc / 1e6, 1),
                        "full_share_of_copy_rate": round(bf / full / 1e6 / (COPY_RATE / 1e12), 3),
                        "compact_share_of_copy_rate": round(bc / comp / 1e6 / (COPY_RATE / 1e12), 3)}
    for e in es:
        e.close()
    return out


def update(a):
    """both creation orders: the streams of the engine created second may share a hardware queue with the caller's stream, which
    serialises its side-stream work (seen in the kernel trace), so each order is timed and the engines are compared in the same place"""
    B, n, steps = a.B_update, 512, 32
    out = {"mode": "update", "B": B, "precision": "bf16", "rows": n * steps}
    for compact_first in (False, True):
        es, *_ = rings(n, steps, max(n, B), compact_first=compact_first)
        g = torch.Generator(device="cuda"); g.manual_seed(2)
        P = 0.02 * torch.randn(es[0].get_buffer("params").numel(), device="cuda", generator=g)
        for e in es:
            e.set_params(P); e.set_params(P, target=True)
        idx = torch.randint(0, n * steps, (B,), dtype=torch.int32, device="cuda")
        isw = torch.ones(B, device="cuda")
        fns = [lambda e=e: e.update_from_replay(idx, isw, gamma=0.99) for e in es]
        full, comp = alternate(fns, a.reps)
        tag = "compact_first" if compact_first else "full_first"
        out[tag] = {"full_us": round(full, 1), "compact_us": round(comp, 1)}
        out.setdefault("full_ring_bytes", es[0].replay_bytes()); out.setdefault("compact_ring_bytes", es[1].replay_bytes())
        for e in es:
            e.close()
        torch.cuda.synchronize()
    f, c = out["full_first"]["full_us"], out["compact_first"]["compact_us"]
    out["ratio_each_created_first"] = round(c / f, 3)
    out["ratio_each_created_second"] = round(out["full_first"]["compact_us"] / out["compact_first"]["full_us"], 3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["observe", "gather", "update", "all"])
    ap.add_argument("--n", type=int, default=512); ap.add_argument("--B", default="512,8192"); ap.add_argument("--B-update", dest="B_update", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compact_probe needs the GPU")
    for m, f in (("observe", observe), ("gather", gather), ("update", update)):
        if a.mode in (m, "all"):
            print(json.dumps(f(a)), flush=True)
