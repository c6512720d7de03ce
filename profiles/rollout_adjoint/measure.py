"""Times of the rollout adjoint and of what is built on it (profiles/rollout_adjoint/README.md).

    python profiles/rollout_adjoint/measure.py [--reps 30] [--warmup 5] [--out FILE]

Shape: bench config 2's nets (quadrotor, E 7, members 200 wide), the bench's scene (synthetic
replay, steady model: every row lives the horizon), model_noise=False, K = H = 10, member 0, at
512 and 4096 rows. Each repetition runs the variants in turn (interleaved); median and p10-p90
over the repetitions after the warm-up ones.

  vjp_fused / vjp_steps   ops.rollout_vjp(path=) between two events on the stream, behind a filler
                          launch that lets the host enqueue ahead of the device, so that the
                          figure is device time (the per-step path's 20 launches and its torch
                          ops included) and not the host's enqueue
  horizon_kernel_KH       the given-actions horizon kernel of the same rows, by the library's own
                          event pair around it (profiles/imagine_actions)
  value_gradient          SMBPO.value_gradient whole, host included (events around the call)
  plan_4 / plan_4_refine_2   plan(iterations=4) without and with refine=2, P = rows / 64 states x 64

FLOPs of the adjoint, per row and step: the forward of trunk L1, trunk L2 and the head's hidden
layer, 2 ((S + A) Hm + 2 Hm^2), and the four backward-data products, 2 ((S + 1) Hm + 2 Hm^2 +
Hm (S + A)): 336,400 at S 12, A 2, Hm 200."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'profiles', 'plan'))
import bench  # noqa: E402
import drpo_amd  # noqa: E402
from drpo_amd import ops  # noqa: E402
from measure import scene, stats, timed  # noqa: E402  (profiles/plan/measure.py)

H, N = 10, 64


def adjoint_flop(S, A, Hm):
    return 2 * ((S + A) * Hm + 2 * Hm * Hm) + 2 * ((S + 1) * Hm + 2 * Hm * Hm + Hm * (S + A))


def timed_ahead(fn, filler):
    """Device time of fn's launches: a filler keeps the device busy while the host enqueues them."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(filler, filler)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def measure(B, reps, warmup):
    dev = torch.device('cuda', 0)
    alg = scene(dev, B, H)
    S, A, Hm = alg.state_dim, alg.action_dim, alg.model_ensemble.hidden_dim
    noise = drpo_amd.DeviceNoise(1)
    run = dict(members=0, deterministic=True, model_noise=False, noise=noise)
    P = B // N
    states = alg.replay_buffer.get('states')[:P].clone()
    tiled = states.repeat_interleave(N, dim=0)
    g = torch.Generator(device=dev).manual_seed(0)
    cand = torch.rand(B, H, A, device=dev, generator=g) * 2 - 1
    im = alg.imagine(tiled, horizon=H, actions=cand, **run)
    torch.cuda.synchronize()
    assert int(im.lengths.min()) == H, 'steady mode: every row lives the horizon'
    gs = torch.randn(B, H + 1, S, device=dev, generator=g)
    gr = torch.randn(B, H, device=dev, generator=g)
    args = ops._vjp_inputs(alg, im, gs, gr)
    filler = torch.randn(6144, 6144, device=dev)
    tmr = ops.EventTimer(2)
    out = {k: getattr(im, k) for k in ops.ImaginedRollout.TENSORS}

    def horizon_kernel():
        ops.rollout_trajectories(alg, alg.actor, tiled, noise, members=0, actions=cand, out=out, timer=tmr, horizon=H)
        torch.cuda.synchronize()
        return tmr.elapsed_pairs(1)[0]

    times = {}
    for rep in range(warmup + reps):
        t = {}
        t['vjp_fused'], f = timed_ahead(lambda: ops._vjp_fused(alg, *args), filler)
        t['vjp_steps'], s = timed_ahead(lambda: ops._vjp_steps(alg, *args), filler)
        t['horizon_kernel_KH'] = horizon_kernel()
        t['value_gradient'], vg = timed(lambda: alg.value_gradient(tiled, cand, horizon=H, members=0, noise=noise))
        t['plan_4'], _ = timed(lambda: alg.plan(states, H, candidates=N, iterations=4, members=0, noise=noise))
        t['plan_4_refine_2'], res = timed(lambda: alg.plan(states, H, candidates=N, iterations=4, members=0,
                                                           noise=noise, refine=2))
        if rep >= warmup:
            for k, v in t.items():
                times.setdefault(k, []).append(v)
    res = {k: stats(v) for k, v in times.items()}
    flop = B * H * adjoint_flop(S, A, Hm)
    med = res['vjp_fused']['median_us']
    res['shape'] = dict(rows=B, P=P, N=N, H=H, S=S, A=A, Hm=Hm, reps=reps,
                        version=int(drpo_amd._lib.lib().drpo_version()), default_path=ops.VJP_DEFAULT_PATH)
    res['derived'] = dict(
        adjoint_flop_per_row_step=adjoint_flop(S, A, Hm),
        fused_tflops=round(flop / med / 1e6, 2),
        fused_fraction_of_fp32_mfma_peak=round(flop / (med * 1e-6) / (bench.FP32_PEAK_TFLOPS * 1e12), 4),
        fused_over_horizon_kernel=round(med / res['horizon_kernel_KH']['median_us'], 3),
        steps_over_fused=round(res['vjp_steps']['median_us'] / med, 2),
        fused_p90_below_steps_p10=bool(res['vjp_fused']['p90_us'] < res['vjp_steps']['p10_us']),
        max_abs_fused_minus_steps=float((f[0] - s[0]).abs().max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = {f'rows_{B}': measure(B, a.reps, a.warmup) for B in (512, 4096)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
