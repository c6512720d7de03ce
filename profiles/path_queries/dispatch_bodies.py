"""Where the literals of tests/test_gpu_path_dispatch.py came from: that module's bodies run against a
built checkout (argv[1], e.g. of the parent commit; "." for this tree) on a GPU, printing what they return.

    python profiles/path_queries/dispatch_bodies.py <checkout> > dispatch_parent.txt"""
import importlib.util
import os
import sys

tree = os.path.abspath(sys.argv[1])
here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(tree, 'tests'))
sys.path.insert(0, tree)
import torch  # noqa: E402
import drpo_amd  # noqa: E402
assert os.path.dirname(drpo_amd.__file__).startswith(tree), drpo_amd.__file__
spec = importlib.util.spec_from_file_location('dispatch_bodies', os.path.join(here, 'tests', 'test_gpu_path_dispatch.py'))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def plan_of(eng):
    if hasattr(eng, 'fit_plan'):
        return eng.fit_plan()
    from drpo_amd.ensemble_engine import FitPlan      # the parent: fit()'s own lines
    m = eng.m
    S, A, rows = m.state_dim, m.action_dim, m.ensemble_size * m.batch_size
    mb = (eng.buf('fit.s_all', rows, S), eng.buf('fit.a_all', rows, A), eng.buf('fit.t_all', rows, S + 1))
    return FitPlan(eng, None, mb, torch.empty(1, device=eng.dev))


for key in T.SAC_LAUNCHES:
    print('SAC', key, T.sac_launches(*key), flush=True)
for key in T.FIT_PLANS:
    p = plan_of(T.fit_model(*key))
    print('FIT', key, (p.fused, p.fb, p.path), flush=True)
