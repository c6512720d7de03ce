"""The two tails of the fused rollout, bracketed with HIP events in one process:

  traj_full       rollout_traj_kernel with every output
  traj_summaries  rollout_traj_kernel with len, ret, hmax, first_violation, terminated only
  emit            the ordered emit of the same staging into the virtual buffer
                  (rollout_emit_self_kernel while H x tiles <= 8192, else rollout_scan +
                  rollout_emit + rollout_persist_finalize)

Each figure is the time from the library's event after rollout_persist_kernel
(step_events[1]) to an event recorded right after the call returns, i.e. the tail's
launches on an otherwise idle stream. The scene is bench.py's (quadrotor, E 7, steady
mode: almost every row lives the whole horizon, so both tails move H x B rows). The
three variants are interleaved, REPS times each; medians and the spread are reported.

  python profiles/imagine/measure.py --out profiles/imagine/measure.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import drpo_amd  # noqa: E402
from drpo_amd import _abi, _lib, ops  # noqa: E402

DEV = torch.device('cuda')
SHAPES = [(4096, 10), (65536, 80)]
SUMMARIES = ('len', 'weights', 'ret', 'hmax', 'first_violation', 'terminated')


def measure(B, H, reps):
    L = _lib.lib()
    alg = bench.make_alg(DEV, B, H, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(0), DEV, alg.env_params)
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    tmr = ops.EventTimer(4)
    noise = drpo_amd.DeviceNoise(0)
    S, A, C = alg.state_dim, alg.action_dim, alg.con_dim

    # one call through the public path fills the cached descriptor; the timed calls go
    # through the C ABI with the library's events switched on and a chosen set of outputs
    w = np.power(np.float64(0.99), np.arange(H, dtype=np.float64))
    im = ops.rollout_trajectories(alg, alg.actor, None, noise, weights=w)
    wdev = torch.as_tensor(w).to(DEV)
    d = ops._rollout_static(alg, alg.actor, B, H, buffer=False)[0]
    d.step_events = tmr.events
    full = _abi.RolloutTraj()
    full.len, full.states, full.actions, full.rewards = (x.data_ptr() for x in (im.lengths, im.states, im.actions,
                                                                                im.rewards))
    full.constraint_values, full.dones, full.violations = (x.data_ptr() for x in (im.constraint_values, im.dones,
                                                                                  im.violations))
    full.weights = wdev.data_ptr()
    full.ret, full.hmax, full.first_violation, full.terminated = (x.data_ptr() for x in (
        im.returns, im.max_constraint, im.first_violation, im.terminated))
    summ = _abi.RolloutTraj()
    for f in SUMMARIES:
        setattr(summ, f, getattr(full, f))

    def tail_ms():
        _lib.check(L.drpo_event_record(tmr.events[2], _lib.stream()), 'event_record')
        torch.cuda.synchronize()
        ms = ctypes.c_float()
        _lib.check(L.drpo_event_elapsed_ms(ctypes.byref(ms), tmr.events[1], tmr.events[2]), 'elapsed')
        return ms.value * 1e3, tmr.elapsed_pairs(1)[0] * 1e3

    def traj(t):
        _lib.check(L.drpo_rollout_trajectories(ctypes.byref(d), ctypes.byref(t), _lib.stream()), 'traj')
        return tail_ms()

    def emit():
        alg.rollout(alg.actor, noise=noise, timer=tmr)
        return tail_ms()

    runs = {'traj_full': lambda: traj(full), 'traj_summaries': lambda: traj(summ), 'emit': emit}
    for f in runs.values():          # warm-up
        for _ in range(3):
            f()
    us = {k: [] for k in runs}
    persist = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            tail, per = f()
            us[k].append(tail)
            persist[k].append(per)
    n = int(im.lengths.sum())
    row_bytes = 4 * (2 * S + A + C + 1) + 2       # one staged transition: s, s2, a, h, r, done | violation bits
    rpt = 32 if B >= 8192 else 16                 # the library's tile choice at quadrotor dims
    self_emit = H * ((B + rpt - 1) // rpt) <= 8192
    res = {'B': B, 'H': H, 'reps': reps, 'transitions': n, 'staged_bytes_per_transition': row_bytes,
           'emit_tail': 'rollout_emit_self' if self_emit else 'rollout_scan + rollout_emit + rollout_persist_finalize'}
    for k in runs:
        a = np.asarray(us[k])
        res[k] = {'median_us': float(np.median(a)), 'min_us': float(a.min()), 'p90_us': float(np.quantile(a, 0.9)),
                  'persist_median_us': float(np.median(persist[k]))}
    res['traj_full_over_emit'] = res['traj_full']['median_us'] / res['emit']['median_us']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    out = []
    for B, H in SHAPES:
        r = measure(B, H, args.reps if B * H < 10 ** 6 else max(5, args.reps // 3))
        print(json.dumps(r), flush=True)
        out.append(r)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
