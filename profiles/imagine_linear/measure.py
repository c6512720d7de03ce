"""The horizon kernel under the linear shield, bracketed with the library's HIP event pair
(step_events, around rollout_persist_kernel) in one process, the variants interleaved:

  P       drpo_rollout_trajectories: no shield
  SHhi    the threshold shield at +inf: one certificate pass, no safe actor
  LINhi   linear, K = 11, +inf: one pass, no safe actor (the early exit)
  LINlo   linear, K = 11, -inf: 10 passes and the safe actor in every tile, the worst case
  LINmid  linear, K = 11, at the median step-0 certificate

each with the distributional certificate (shield_uncertainty=True, the threshold shield's
default here, so SHhi and LINhi run the same certificate) and, suffix _m, with the mean
certificate (the linear shield's default). The scene is bench.py's (quadrotor, E 7, steady
mode: every row lives the whole horizon). REPS times each after a warm-up; medians and the
spread are reported. The large shape runs once each after one warm-up round.

A tile runs as many certificate passes as its slowest row needs: min(max_j + 1, K-1) with
max_j the largest blend index among its rows, and the safe actor if max_j > 0. The FLOP of
a variant are counted from its own blend output that way.

  python profiles/imagine_linear/measure.py --large --out profiles/imagine_linear/measure.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import drpo_amd  # noqa: E402
from drpo_amd import ops  # noqa: E402

DEV = torch.device('cuda')
K = 11
INF = float('inf')
# per transition: DESIGN §4's formula; one certificate pass (both heads / the mean head); the safe actor
FLOP_BASE, FLOP_CERT, FLOP_CERT_MEAN, FLOP_SAFE = 395264, 402432, 270336, 139264
PEAK_FP32_MFMA = bench.FP32_PEAK_TFLOPS * 1e12
# name: (threshold or 'mid', candidates, shield_uncertainty)
VARIANTS = {'P': None,
            'SHhi': (INF, None, True), 'LINhi': (INF, K, True), 'LINlo': (-INF, K, True), 'LINmid': ('mid', K, True),
            'SHhi_m': (INF, None, False), 'LINhi_m': (INF, K, False), 'LINlo_m': (-INF, K, False),
            'LINmid_m': ('mid', K, False)}


def passes_and_safe(im, rpt):
    """(certificate passes, safe-actor runs) per tile and step, averaged, from a run's outputs."""
    if im.blend is None:
        j = im.interventions.to(torch.int64)
        top = 1
    else:
        j = im.blend.to(torch.int64)
        top = im.shield_candidates - 1
    B, H = j.shape
    pad = (-B) % rpt
    jm = torch.nn.functional.pad(j, (0, 0, 0, pad)).reshape(-1, rpt, H).max(1)[0]       # [tiles, H]
    return float(torch.clamp(jm + 1, max=top).float().mean()), float((jm > 0).float().mean())


def measure(B, H, reps, warm):
    alg = bench.make_alg(DEV, B, H, 7, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(0), DEV, alg.env_params)
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    alg.model_ensemble.state_normalizer.fit(alg.replay_buffer.get('states'))
    bench.steady_mode(alg)
    assert alg.solver.distributional_qc
    rpt = 32 if B >= 8192 else 16
    tmr = ops.EventTimer(2)
    noise = drpo_amd.DeviceNoise(0)
    im = ops.rollout_trajectories(alg, alg.actor, None, noise)
    torch.cuda.synchronize()
    assert int(im.lengths.min()) == H, 'steady mode: every row lives the horizon'
    out = {k: getattr(im, k) for k in ops.ImaginedRollout.TENSORS}
    mid, work = {}, {}

    def run(name):
        v = VARIANTS[name]
        kw = {}
        if v is not None:
            thr, cand, unc = v
            kw = dict(shield=mid[unc] if thr == 'mid' else thr, shield_candidates=cand, shield_uncertainty=unc)
        r = ops.rollout_trajectories(alg, alg.actor, None, noise, out=out, timer=tmr, **kw)
        torch.cuda.synchronize()
        if v is not None and name not in work:
            work[name] = passes_and_safe(r, rpt)
            if name.startswith('LINhi'):
                mid[v[2]] = float(r.certificate[:, 0].median())
        return tmr.elapsed_pairs(1)[0] * 1e3       # us

    for _ in range(warm):
        for name in VARIANTS:
            run(name)
    us = {name: [] for name in VARIANTS}
    for _ in range(reps):
        for name in VARIANTS:
            us[name].append(run(name))
    for name in ('SHhi', 'LINhi', 'SHhi_m', 'LINhi_m'):
        assert work[name] == (1.0, 0.0), (name, work[name])
    for name in ('LINlo', 'LINlo_m'):
        assert work[name] == (K - 1.0, 1.0), (name, work[name])
    res = {'B': B, 'H': H, 'reps': reps, 'transitions': B * H, 'rows_per_tile': rpt,
           'threshold_mid': {'distributional': mid[True], 'mean': mid[False]}}
    for name, v in VARIANTS.items():
        a = np.asarray(us[name])
        per = FLOP_BASE
        if v is not None:
            p, s = work[name]
            per += p * (FLOP_CERT if v[2] else FLOP_CERT_MEAN) + s * FLOP_SAFE
        flop = B * H * per
        med = float(np.median(a))
        res[name] = {'median_us': med, 'min_us': float(a.min()), 'max_us': float(a.max()),
                     'p10_us': float(np.quantile(a, 0.1)), 'p90_us': float(np.quantile(a, 0.9)),
                     'passes_per_tile_step': None if v is None else work[name][0],
                     'safe_actor_per_tile_step': None if v is None else work[name][1],
                     'flop_per_transition': per, 'algorithmic_tflops': flop / med / 1e6,
                     'fraction_of_fp32_mfma_peak': flop / (med * 1e-6) / PEAK_FP32_MFMA}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--large', action='store_true', help='also B 65536, H 80, one run each')
    args = ap.parse_args()
    out = [measure(4096, 10, args.reps, 3)]
    print(json.dumps(out[-1]), flush=True)
    if args.large:
        torch.cuda.empty_cache()
        out.append(measure(65536, 80, 1, 1))
        print(json.dumps(out[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
