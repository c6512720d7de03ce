"""The path queries of include/drpo_hip.h (drpo_mlp_pair_ok .. drpo_rollout_engine,
drpo_abi_const), no GPU. A fused launch's shape condition is written once, in
csrc/path_shapes.hpp; the entry point refuses by it and the Python engines pick their path by
asking the query. Here:

  1. each query against a table of shapes (tests/path_query_tables.py) and a literal list of
     verdicts. The lists are what the Python predicates of the commit before the queries
     (mlp_desc.pairable, SACEngine._ccb_fused / _post_mult / _fb_actor,
     ensemble_engine.ens_fused_shapes / ens_fb_shapes) said for the same tables
     (profiles/path_queries/parent_verdicts.py prints them), but for the two post-chain cases
     the table itself explains;
  2. query and entry point agree: a rows = 0 call (accepted before any launch) is accepted
     exactly when the query says yes; drpo_mlp_backward_ens and drpo_ens_fit_fb cannot accept
     without launching, so there only: query 0 -> DRPO_EINVAL with the entry point's message;
  3. every constant Python mirrors equals drpo_abi_const of its name;
  4. drpo_rollout_engine over descriptors with dummy pointers.
Pointers are dummies the host never dereferences."""
import ctypes

import pytest

from drpo_amd import _abi, _lib, envs, mlp_desc, ops, optim
import path_query_tables as T
from test_mlp_desc_checks import EINVAL, OK, P, PAIR_SHAPES, R3, RELU, TANH, NONE, _actor_head, _bwd_job, _err, \
    _fwd_job, _fwd_net, _multi
from test_ens_desc_checks import _red, _up

ref = ctypes.byref


def _net(net):
    d = _abi.MlpNet()
    _fwd_net(d, *net)
    return d


def _fwd_multi(job):
    return _multi(_lib.lib().drpo_mlp_forward_multi, [job], 0, 0)


# ------------------------------------------------------------------ pair jobs
PAIR = [(s, s) for s in PAIR_SHAPES] + [(PAIR_SHAPES[0], ([16, 256, 256, 4], R3)),
                                        (PAIR_SHAPES[0], ([16, 256, 256, 6], [RELU, TANH, NONE]))]
# (the list of test_mlp_desc_checks.test_pairable_agrees_with_the_c_pair_check, which holds
# mlp_desc.pairable and the entry point together over the same cases)
PAIR_WANT = [True, False, False, True, True, False, False, False, True, False, False, False, False, False, False,
             False]


def test_pair_query_table():
    L = _lib.lib()
    assert [bool(L.drpo_mlp_pair_ok(ref(_net(a)), ref(_net(b)))) for a, b in PAIR] == PAIR_WANT
    for (a, b), want in zip(PAIR, PAIR_WANT):
        assert _fwd_multi(_fwd_job([a, b], a[0][0], pair=1)) == (OK if want else EINVAL), (a, b, _err())


# ------------------------------------------------------------------ paired heads (ccb_out)
def heads_query(L, case):
    return bool(L.drpo_mlp_heads_paired(*[ref(_net(n)) for n in case]))


def heads_entry(L, case):
    """rows = 0 drpo_mlp_forward_multi of the trunk job with the constraint bound requested"""
    job = _fwd_job(list(case), case[0][0][0], trunk=1)
    job.ccb_out = P
    return _fwd_multi(job)


def test_heads_query_table():
    L = _lib.lib()
    assert [heads_query(L, c) for c in T.HEADS] == T.HEADS_WANT
    assert any(T.HEADS_WANT) and not all(T.HEADS_WANT)


@pytest.mark.parametrize('i', range(len(T.HEADS)))
def test_heads_query_is_the_entry_points_verdict(i):
    L = _lib.lib()
    want = heads_query(L, T.HEADS[i])
    assert heads_entry(L, T.HEADS[i]) == (OK if want else EINVAL), _err()
    if not want:
        assert 'drpo_mlp_forward_multi: job 0: the constraint bound needs a trunk job with paired heads' in _err()


# ------------------------------------------------------------------ post chain
def post_query(L, case):
    S, A, post = case
    return bool(L.drpo_mlp_post_ok(S, ref(_net(post))))


def post_entry(L, case):
    """rows = 0 drpo_mlp_forward_multi of the reference certificate job on [s (S), a (A)] with
    its bound and the post chain"""
    S, A, post = case
    job = _fwd_job([([S + A, 256, 256], T.RR), T.HEAD, T.HEAD], S, trunk=1)
    job.src[1], job.cols[1], job.ld[1] = P, A, A
    job.ccb_out = P
    _fwd_net(job.post, *post)
    return _fwd_multi(job)


def test_post_query_table():
    L = _lib.lib()
    assert [post_query(L, c) for c in T.POST] == T.POST_WANT
    # where the list departs from the parent's Python predicate (the table says why)
    assert [i for i, (a, b) in enumerate(zip(T.POST_WANT, T.POST_PARENT_PYTHON)) if a != b] == [4, 5]


@pytest.mark.parametrize('i', range(len(T.POST)))
def test_post_query_is_the_entry_points_verdict(i):
    L = _lib.lib()
    want = post_query(L, T.POST[i])
    assert post_entry(L, T.POST[i]) == (OK if want else EINVAL), _err()
    if not want:
        assert 'drpo_mlp_forward_multi: job 0: a post chain needs the job\'s constraint bound' in _err()


# ------------------------------------------------------------------ fused actor pass
def fb_query(L, case):
    S, *nets, C = case
    return bool(L.drpo_mlp_fb_ok(S, *[ref(_net(n)) for n in nets], C))


def fb_entry(L, case):
    """drpo_mlp_fb_multi with actor.B = 0 over the actor update's three jobs (sac_step.py
    'a.fb'): [certificate + bound + multiplier post chain, certificate], certificate, Q_k for
    each of q0 / q1. OK only when both launches are accepted; else the first refusal."""
    S, trunk, h1, h2, post, q0, q1, C = case
    A = trunk[0][0] - S
    for q in (q0, q1):
        def cc():
            job = _fwd_job([trunk, h1, h2], S, trunk=1)
            job.src[1], job.cols[1], job.ld[1] = P, A, A
            return job
        ccm = cc()
        ccm.ccb_out = P
        _fwd_net(ccm.post, *post)
        qj = _fwd_job([q], S)
        qj.src[1], qj.cols[1], qj.ld[1] = P, A, A
        fw = [ccm, cc(), cc(), qj]
        bw = [_bwd_job([trunk, h1, h2], trunk=1, upstream=mlp_desc.UPSTREAM_ACTOR_CC, gout=0),
              _bwd_job([trunk, h1, h2], trunk=1, upstream=mlp_desc.UPSTREAM_SAFE_CC, gout=0),
              _bwd_job([q], upstream=mlp_desc.UPSTREAM_NEG_MEAN, gout=0)]
        h = _actor_head()
        h.C, h.lams = C, P
        fa, ba, ja = (_abi.MlpFwd * 4)(*fw), (_abi.MlpBwd * 3)(*bw), (_abi.MlpFbJob * 3)()
        for J, (fi, bi) in zip(ja, [((0, 1), 0), ((2,), 1), ((3,), 2)]):
            J.nfwd, J.bwd = len(fi), bi
            for k, f in enumerate(fi):
                J.fwd[k] = f
        rc = L.drpo_mlp_fb_multi(fa, P, 4, ba, P, 3, ja, 3, ref(h), 0, 0, None)
        if rc != OK:
            return rc
    return OK


def test_fb_query_table():
    L = _lib.lib()
    assert [fb_query(L, c) for c in T.FB] == T.FB_WANT
    assert any(T.FB_WANT) and not all(T.FB_WANT)


@pytest.mark.parametrize('i', range(len(T.FB)))
def test_fb_query_is_the_entry_points_verdict(i):
    L = _lib.lib()
    want = fb_query(L, T.FB[i])
    assert fb_entry(L, T.FB[i]) == (OK if want else EINVAL), _err()
    if not want:
        assert _err().startswith('drpo_mlp_fb_multi: ')


# ------------------------------------------------------------------ model fit
def fit_descs(case, Z=7, b=256):
    """The split-heads descriptors of a fit step (forward, backward, NLL upstream) over the
    case's trunk and heads, with every pointer the entry points require."""
    S, A, *nets = case
    f, bd = _abi.MlpFwd(), _abi.MlpBwd()
    f.src[0] = f.src[1] = P
    f.cols[0], f.cols[1], f.ld[0], f.ld[1] = S, A, S, A
    for j, (dims, acts) in enumerate(nets):
        f.net[j].nl = bd.net[j].nl = len(dims) - 1
        for l in range(len(dims) - 1):
            fl, bl = f.net[j].L[l], bd.net[j].L[l]
            fl.W, fl.b, fl.din, fl.dout, fl.act = P, P, dims[l], dims[l + 1], acts[l]
            bl.W, bl.din, bl.dout, bl.act, bl.dz = P, dims[l], dims[l + 1], acts[l], P
            if j == 0:
                bl.dz2 = P
    f.nnets = bd.nnets = 3
    f.trunk = bd.trunk = f.split_heads = bd.split_heads = 1
    f.rows = bd.rows = b
    f.nbatch = bd.nbatch = Z
    bd.upstream = mlp_desc.UPSTREAM_ENS
    return f, bd, _up(S=S, Z=Z, b=b)


def fit_paths(L, case):
    f, bd, up = fit_descs(case)
    return L.drpo_ens_fit_paths(ref(f), ref(bd), ref(up))


def test_fit_paths_tables():
    L = _lib.lib()
    assert [bool(fit_paths(L, c) & 1) for c in T.ENS_BWD] == T.ENS_BWD_WANT
    assert [bool(fit_paths(L, c) & 2) for c in T.ENS_FB] == T.ENS_FB_WANT
    assert fit_paths(L, T.ENS_BWD[0]) == 3      # the reference model takes the one-launch step


@pytest.mark.parametrize('i', [i for i, w in enumerate(T.ENS_BWD_WANT) if not w])
def test_backward_ens_refuses_what_the_query_refuses(i):
    L = _lib.lib()
    f, bd, up = fit_descs(T.ENS_BWD[i])
    assert not L.drpo_ens_fit_paths(ref(f), ref(bd), ref(up)) & 1
    out = _abi.EnsReduce()
    assert L.drpo_mlp_backward_ens(ref(bd), ref(up), ref(_red(S1=up.S + 1)), ref(out), None) == EINVAL
    assert _err() == 'drpo_mlp_backward_ens: ' + T.ENS_BWD_REFUSAL.get(i, T.ENS_BWD_REFUSAL_DEFAULT)


@pytest.mark.parametrize('i', [i for i, w in enumerate(T.ENS_FB_WANT) if not w])
def test_fit_fb_refuses_what_the_query_refuses(i):
    L = _lib.lib()
    f, bd, up = fit_descs(T.ENS_FB[i])
    assert not L.drpo_ens_fit_paths(ref(f), ref(bd), ref(up)) & 2
    out = _abi.EnsReduce()
    assert L.drpo_ens_fit_fb(ref(f), ref(bd), ref(up), ref(_red(S1=up.S + 1)), ref(out), None) == EINVAL
    assert _err().startswith('drpo_ens_fit_fb: needs the ensemble trunk [S+A <= 64 -> H -> H] and two heads')


def test_queries_refuse_null_descriptors():
    L = _lib.lib()
    n = ref(_net(T.Q))
    assert L.drpo_mlp_pair_ok(None, n) == 0 and L.drpo_mlp_heads_paired(n, None, n) == 0
    assert L.drpo_mlp_post_ok(12, None) == 0 and L.drpo_mlp_fb_ok(12, n, n, n, n, n, None, 2) == 0
    assert L.drpo_ens_fit_paths(None, None, None) == 0 and L.drpo_rollout_engine(None) == 0


# ------------------------------------------------------------------ constants
def test_python_mirrors_equal_the_librarys_constants():
    c = lambda name: _lib.lib().drpo_abi_const(name.encode())
    A = mlp_desc.ACT_ID
    mirrors = {
        'DRPO_ACT_NONE': A[None], 'DRPO_ACT_RELU': A['relu'], 'DRPO_ACT_SILU': A['swish'], 'DRPO_ACT_TANH': A['tanh'],
        'DRPO_HEAD_SAMPLE': mlp_desc.HEAD_SAMPLE, 'DRPO_HEAD_RSAMPLE': mlp_desc.HEAD_RSAMPLE,
        'DRPO_HEAD_MEAN': mlp_desc.HEAD_MEAN,
        'DRPO_ROLLOUT_FUSED_MAX_H': ops.TRAJ_MAX_H, 'DRPO_OPTIM_MAX_SEGS': optim.OPT_MAXSEG,
        'DRPO_PROG_MAX_ROWS': _abi.PROG_MAX_ROWS, 'DRPO_PROG_MAX_TERMS': _abi.PROG_MAX_TERMS,
        'DRPO_PROG_MAX_CENTRES': _abi.PROG_MAX_CENTRES, 'DRPO_PROG_MAX_BOX': _abi.PROG_MAX_BOX,
        'DRPO_PROG_AFFINE': _abi.PROG_AFFINE, 'DRPO_PROG_BALLS': _abi.PROG_BALLS,
        'DRPO_ENV_PROGRAM': _abi.ENV_PROGRAM,
        'DRPO_ENV_POINT_ROBOT': envs.ENV_NAMES['point-robot'], 'DRPO_ENV_QUADROTOR': envs.ENV_NAMES['quadrotor'],
        'DRPO_ENV_CARTPOLE': envs.ENV_NAMES['cartpole'], 'DRPO_ENV_TRACKING': envs.ENV_NAMES['tracking'],
    }
    for name in ('GOUT', 'CRITIC', 'CERT', 'ENS', 'ACTOR_CC', 'SAFE_CC', 'NEG_MEAN', 'SQUASH', 'SQUASH_SAFE'):
        mirrors['DRPO_UPSTREAM_' + name] = getattr(mlp_desc, 'UPSTREAM_' + name)
    for name, value in mirrors.items():
        assert c(name) == value, name
    assert A['identity'] == A[None]
    assert envs.ENV_PROGRAM == _abi.ENV_PROGRAM
    assert sorted(envs.ENV_IDS.values()) == [c('DRPO_ENV_POINT_ROBOT'), c('DRPO_ENV_QUADROTOR'),
                                             c('DRPO_ENV_CARTPOLE'), c('DRPO_ENV_TRACKING')]
    P_ = envs.ConstraintProgram
    assert (P_.MAX_ROWS, P_.MAX_TERMS, P_.MAX_CENTRES, P_.MAX_BOX) == tuple(
        c('DRPO_PROG_MAX_' + k) for k in ('ROWS', 'TERMS', 'CENTRES', 'BOX'))
    # the launch limits that only the library reads
    assert (c('DRPO_MLP_MULTI_MAX_JOBS'), c('DRPO_MLP_MULTI_MAX_SLOTS'), c('DRPO_MLP_FB_MAX_JOBS')) == (8, 16, 4)
    assert c('DRPO_NO_SUCH_CONSTANT') == -1 and c('') == -1


# ------------------------------------------------------------------ rollout engine
@pytest.mark.parametrize('case, want', T.ROLLOUT)
def test_rollout_engine(case, want):
    engine, draws, layout, H = case
    d = _abi.RolloutDesc()
    d.engine, d.eps_layout, d.H = engine, layout, H
    d.eps_a = d.eps_m = P if draws else None
    assert _lib.lib().drpo_rollout_engine(ref(d)) == want
