"""Where the literal verdict lists of tests/path_query_tables.py came from: the Python
predicates of the commit before the path queries, evaluated on this tree's tables, next to
what that commit's entry points said for the same cases (rows = 0 calls, no GPU).

    python profiles/path_queries/parent_verdicts.py <built checkout of the parent commit>

The rollout table has no parent function to call (the rule was inline in ops.rollout:
``1 if (noise.parity and eps_layout == 0) or H > 128 else 2``)."""
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
parent = os.path.abspath(sys.argv[1])
sys.path.insert(0, parent)
import drpo_amd                                                    # noqa: E402  (the parent's package)
assert os.path.dirname(drpo_amd.__file__).startswith(parent)
from drpo_amd import _lib, mlp_desc                                # noqa: E402
from drpo_amd.ensemble_engine import ens_fb_shapes, ens_fused_shapes   # noqa: E402
from drpo_amd.sac_step import SACEngine                            # noqa: E402

sys.path.insert(0, os.path.join(HERE, '..', '..', 'tests'))
import path_query_tables as T                                      # noqa: E402
import test_path_queries as Q                                      # noqa: E402  (its descriptor builders only)


class _T:
    def data_ptr(self):
        return 0x1000


def net(n):
    dims, acts = n
    return mlp_desc.Net([(_T(), _T(), dims[l], dims[l + 1], acts[l], None) for l in range(len(dims) - 1)])


def engine(S, trunk, h1, h2, mult=None, q0=T.Q, q1=T.Q):
    e = object.__new__(SACEngine)
    e.S, e.cost, e.post_mult, e.fb_actor = S, False, True, True
    e.sol = SimpleNamespace(mlp_multiplier=True)
    e.nets = {'cc_trunk': net(trunk), 'cc_mean': net(h1), 'cc_ls': net(h2), 'q0': net(q0), 'q1': net(q1)}
    if mult is not None:
        e.nets['mult'] = net(mult)
    return e


L = _lib.lib()
ok = lambda rc: rc == 0
show = lambda name, python, entry: print(f'{name}\n  parent python: {python}\n  parent entry : {entry}')

show('PAIR', [mlp_desc.pairable(net(a), net(b)) for a, b in Q.PAIR],
     [ok(Q._fwd_multi(Q._fwd_job([a, b], a[0][0], pair=1))) for a, b in Q.PAIR])
show('HEADS', [bool(engine(12, *c)._ccb_fused()) for c in T.HEADS], [ok(Q.heads_entry(L, c)) for c in T.HEADS])
show('POST', [bool(engine(S, ([S + A, 256, 256], T.RR), T.HEAD, T.HEAD, post)._post_mult()) for S, A, post in T.POST],
     [ok(Q.post_entry(L, c)) for c in T.POST])
show('FB', [bool(engine(S, t, h1, h2, post, q0, q1)._fb_actor(True)) for S, t, h1, h2, post, q0, q1, C in T.FB],
     [ok(Q.fb_entry(L, c)) for c in T.FB])
show('ENS_BWD', [bool(ens_fused_shapes([net(n) for n in nets], S + 1)) for S, A, *nets in T.ENS_BWD],
     'launches when it accepts: see tests/test_path_queries.py for the refusing direction')
show('ENS_FB', [bool(ens_fb_shapes([net(n) for n in nets], S, A)) for S, A, *nets in T.ENS_FB],
     'launches when it accepts: see tests/test_path_queries.py for the refusing direction')
