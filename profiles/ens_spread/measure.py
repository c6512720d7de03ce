"""drpo_ens_spread against its yardsticks, in one process with HIP events, the variants
interleaved, REPS times each after a warm-up; medians and p10-p90.

Workload: bench.py's quadrotor model (S 12, A 2, E 7, hidden 200) on n = 40,960 replay rows
(config 2's B * H).

  kernel   on the raw head outputs D / LVR of ONE all-member forward:
             head7      drpo_ens_head, all 7 members, mu + lv outputs (the yardstick: it reads
                        the same arrays and writes 2 * 7 * n * (S+1) floats)
             spread5    drpo_ens_spread, the 5 elites, all six outputs
             spread7    the same over all 7 members (zsel NULL)
             spread5r   the 5 elites, the three per-row outputs alone
           and, on synthetic D / LVR of 32 members (the pair loop's 496 pairs per row):
             head32, spread32
  api      model.means(s, a) against model.disagreement(s, a) (elites) and
           model.disagreement(s, a, members='all'): the same forward in front of each
  large    (--large) one run: n = 65536 * 80 rows through the chunking, E 32 if it fits;
           time and peak workspace

  python profiles/ens_spread/measure.py --large --out profiles/ens_spread/measure.json
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
import drpo_amd  # noqa: E402,F401
from drpo_amd import _abi, _lib  # noqa: E402

DEV = torch.device('cuda')
N = 40960
OUTPUTS = ('mean', 'epistemic_std', 'aleatoric_std', 'disagreement', 'epistemic', 'aleatoric')


def scene(E, rows):
    alg = bench.make_alg(DEV, 4096, 10, E, 0, bench.QUAD_JSON)
    rep = bench.synth_replay('quadrotor', 100000, np.random.RandomState(0))
    alg.replay_buffer.extend(**{k: torch.from_numpy(v).to(DEV) for k, v in rep.items()})
    m = alg.model_ensemble
    m.state_normalizer.fit(alg.replay_buffer.get('states'))
    m._elite_inds = list(range(min(5, E)))
    s, a = alg.replay_buffer.get('states', 'actions')
    reps = -(-rows // len(s))
    return m, s.repeat(reps, 1)[:rows].contiguous(), a.repeat(reps, 1)[:rows].contiguous()


def stats(us):
    a = np.asarray(us)
    return {'median_us': float(np.median(a)), 'p10_us': float(np.quantile(a, 0.1)),
            'p90_us': float(np.quantile(a, 0.9)), 'min_us': float(a.min()), 'max_us': float(a.max())}


def interleaved(variants, reps, warm):
    """variants: name -> callable that enqueues the work; HIP events around each call"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    us = {k: [] for k in variants}
    for i in range(warm + reps):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= warm:
                us[k].append(ev[0].elapsed_time(ev[1]) * 1e3)
    return {k: stats(v) for k, v in us.items()}


def spread_call(D, LVR, s, lo, hi, n, S, Z, zsel, scale, outputs):
    S1 = S + 1
    bufs = {k: torch.empty((n, S1) if k in OUTPUTS[:3] else (n,), device=DEV) for k in outputs}
    d = _abi.EnsSpread()
    d.D, d.LVR, d.s, d.minlv, d.maxlv = (t.data_ptr() for t in (D, LVR, s, lo, hi))
    d.zsel, d.scale = (None if zsel is None else zsel.data_ptr()), scale.data_ptr()
    d.n, d.S, d.Z, d.M = n, S, Z, Z if zsel is None else len(zsel)
    for k, v in bufs.items():
        setattr(d, k, v.data_ptr())
    L, ref = _lib.lib(), ctypes.byref(d)
    keep = (bufs, d, zsel)

    def run(keep=keep):
        _lib.check(L.drpo_ens_spread(ref, _lib.stream()), 'ens_spread')
    nbytes = 4 * (d.M * n * S1 * (2 if any(k.startswith('alea') for k in outputs) else 1)
                  + (n * S if 'mean' in outputs else 0) + sum(v.numel() for v in bufs.values()))
    return run, nbytes


def head_call(D, LVR, s, lo, hi, n, S, Z):
    mu, lv = torch.empty(Z, n, S + 1, device=DEV), torch.empty(Z, n, S + 1, device=DEV)
    L = _lib.lib()

    def run():
        _lib.check(L.drpo_ens_head(_lib.ptr(D), _lib.ptr(LVR), _lib.ptr(s), 0, n, S, Z, _lib.ptr(lo), _lib.ptr(hi), None,
                                   None, 0, 0, _lib.ptr(mu), _lib.ptr(lv), None, None, _lib.stream()), 'ens_head')
    return run, 4 * (4 * Z * n * (S + 1) + n * S)


def kernels(reps, warm):
    m, s, a = scene(7, N)
    S, E, eng = m.state_dim, m.ensemble_size, m.engine
    nets, _, _ = eng._forward(s, a, N, E, 0, 0)
    D, LVR = nets[1].sy[-1], nets[2].sy[-1]
    lo, hi = m.min_log_var.data, m.max_log_var.data
    scale = torch.cat([1.0 / (m.state_normalizer.std + 1e-6), torch.zeros(1, device=DEV)]).contiguous()
    elites = torch.tensor(m._elite_inds, dtype=torch.int32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    D32 = torch.randn(32, N, S + 1, device=DEV, generator=g)
    L32 = torch.randn(32, N, S + 1, device=DEV, generator=g) * 3 - 5
    calls = {'head7': head_call(D, LVR, s, lo, hi, N, S, E),
             'spread5': spread_call(D, LVR, s, lo, hi, N, S, E, elites, scale, OUTPUTS),
             'spread7': spread_call(D, LVR, s, lo, hi, N, S, E, None, scale, OUTPUTS),
             'spread5r': spread_call(D, LVR, s, lo, hi, N, S, E, elites, scale, OUTPUTS[3:]),
             'head32': head_call(D32, L32, s, lo, hi, N, S, 32),
             'spread32': spread_call(D32, L32, s, lo, hi, N, S, 32, None, scale, OUTPUTS)}
    res = interleaved({k: v[0] for k, v in calls.items()}, reps, warm)
    for k, (_, nbytes) in calls.items():
        res[k]['bytes'] = nbytes
        res[k]['GBps_at_median'] = nbytes / res[k]['median_us'] / 1e3
    api = interleaved({'means': lambda: m.means(s, a), 'disagreement': lambda: m.disagreement(s, a),
                       'disagreement_all': lambda: m.disagreement(s, a, members='all')}, reps, warm)
    return {'n': N, 'S': S, 'E': E, 'reps': reps, 'kernel': res, 'api': api}


def large():
    rows = 65536 * 80
    out = {'rows': rows, 'single_run': True}
    for E in (32, 7):
        try:
            torch.cuda.empty_cache()
            m, s, a = scene(E, rows)
            m.disagreement(s[:4096], a[:4096])                      # code objects loaded, nothing else warm
            torch.cuda.synchronize()
            del m.engine.ws['f.D'], m.engine.ws['f.L']
            torch.cuda.empty_cache()
            res = {}
            for name, members in (('elites', None), ('all', 'all')):
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                sp = m.disagreement(s, a, members=members)
                ev[1].record()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                outputs = sum(getattr(sp, k).numel() * 4 for k in OUTPUTS)
                res[name] = {'ms': ev[0].elapsed_time(ev[1]), 'M': len(sp.members), 'peak_bytes_over_inputs': peak,
                             'output_bytes': outputs, 'workspace_bytes': peak - outputs,
                             'max_disagreement': float(sp.disagreement.max())}
                del sp
            out['E'] = E
            out.update(res)
            return out
        except torch.cuda.OutOfMemoryError as e:
            out[f'E{E}'] = 'out of memory: ' + str(e)[:80]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--large', action='store_true')
    args = ap.parse_args()
    out = {'config2': kernels(args.reps, 3)}
    print(json.dumps(out['config2']), flush=True)
    if args.large:
        out['large'] = large()
        print(json.dumps(out['large']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
