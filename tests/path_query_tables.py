"""The shape tables of tests/test_path_queries.py, as plain data (no import of the package, so
that profiles/path_queries/parent_verdicts.py can evaluate the parent commit's Python
predicates on the very same cases). A net is (dims, acts): layer l is dims[l] -> dims[l + 1]
with activation acts[l].

Every table is anchored at a reference shape and changes one thing at a time:
  SAC, quadrotor (S 12, A 2, C 2): trunk [14, 256, 256], heads [256, 256, 2], critics
  [14, 256, 256, 1], multiplier [13, 256, 256, 1];  model: trunk [14, 200, 200], heads
  [200, 200, 13], swish.
Each has an accepted case and, for every clause of its condition, a case that fails that
clause and no other (the comment of a case names the clause)."""
NONE, RELU, SWISH, TANH = 0, 1, 2, 3
RR, RN, RRN = [RELU, RELU], [RELU, NONE], [RELU, RELU, NONE]
SS, SN = [SWISH, SWISH], [SWISH, NONE]

TRUNK = ([14, 256, 256], RR)
HEAD = ([256, 256, 2], RN)
Q = ([14, 256, 256, 1], RRN)
MULT = ([13, 256, 256, 1], RRN)


def _head(hid=256, out=2, acts=RN, din=256):
    return ([din, hid, out], acts)


# ---- paired heads: (trunk, head 1, head 2)
HEADS = [
    (TRUNK, HEAD, HEAD),                                             # the reference widths
    (([14, 256, 255], RR), _head(din=255), _head(din=255)),          # trunk output 255
    (TRUNK, ([256, 2], [NONE]), HEAD),                               # head 1 of depth 1
    (TRUNK, HEAD, ([256, 2], [NONE])),                               # head 2 of depth 1
    (TRUNK, ([256, 2], [NONE]), ([256, 2], [NONE])),                 # both of depth 1
    (TRUNK, ([256, 256, 256, 2], RRN), ([256, 256, 256, 2], RRN)),   # both of depth 3
    (TRUNK, ([256, 256, 256, 2], RRN), HEAD),                        # head 1 of depth 3
    (TRUNK, _head(200), _head(200)),                                 # hidden 200 / 200
    (TRUNK, _head(256), _head(200)),                                 # hidden 256 / 200
    (TRUNK, _head(out=16), _head(out=16)),                           # output 16
    (TRUNK, _head(out=17), _head(out=17)),                           # output 17
    (TRUNK, _head(out=17), HEAD),                                    # output 17 in head 1 alone
    (TRUNK, HEAD, _head(out=17)),                                    # ... in head 2 alone
    (TRUNK, HEAD, _head(acts=[TANH, NONE])),                         # activations differ in layer 0
    (TRUNK, HEAD, _head(acts=[RELU, TANH])),                         # ... in layer 1
    (TRUNK, _head(acts=[TANH, TANH]), _head(acts=[TANH, TANH])),     # equal activations, not ReLU / identity
]
HEADS_WANT = [True, False, False, False, False, False, False, True, False, True, False, False, False, False, False,
              True]

# ---- post chain behind the bound: (cols0 = S, A, the post net); the job's nets are the
# reference constraint critic on S + A inputs
POST = [
    (12, 2, MULT),                                   # the reference multiplier
    (63, 2, ([64, 256, 256, 1], RRN)),               # cols0 63
    (64, 2, ([65, 256, 256, 1], RRN)),               # cols0 64
    (12, 2, ([12, 256, 256, 1], RRN)),               # first din == cols0, not cols0 + 1
    (12, 2, ([13, 257, 257, 1], RRN)),               # a 257-wide layer
    (12, 2, ([13, 256, 256, 256, 1], [RELU] * 3 + [NONE])),   # four layers
    (12, 2, ([13, 64, 1], RN)),                      # a narrower, shallower net
]
# The parent's SACEngine._post_mult said True for the 257-wide and the four-layer net, and its
# drpo_mlp_forward_multi refused both ("a post chain needs ..."): the two sides had drifted.
# No configuration reached it (every forward refuses such a net first). The query is the
# entry point's condition, so both are False here.
POST_WANT = [True, True, False, False, False, False, True]
POST_PARENT_PYTHON = [True, True, False, False, True, True, True]

# ---- the actor update's fused forward + backward: (cols0, trunk, h1, h2, post, q0, q1, C)


def _fb(trunk=TRUNK, h1=HEAD, h2=HEAD, post=MULT, q0=Q, q1=Q, C=2):
    return (12, trunk, h1, h2, post, q0, q1, C)


FB = [
    _fb(),                                                           # the reference widths
    _fb(h1=_head(200), h2=_head(200)),                               # heads 200 wide: paired, not fused
    _fb(trunk=([14, 256, 256], [TANH, RELU])),                       # a tanh trunk layer
    _fb(h1=_head(acts=[TANH, NONE]), h2=_head(acts=[TANH, NONE])),   # tanh head hidden layers
    _fb(q0=([14, 256, 256, 1], [RELU, TANH, NONE])),                 # a tanh critic hidden layer (q0)
    _fb(q1=([14, 256, 256, 1], [TANH, RELU, NONE])),                 # ... (q1)
    _fb(q0=([14, 16, 256, 1], RRN), q1=([14, 16, 256, 1], RRN)),     # a critic hidden layer 16 wide
    _fb(q0=([14, 17, 256, 1], RRN), q1=([14, 17, 256, 1], RRN)),     # ... 17 wide
    _fb(trunk=([14, 16, 256], RR)),                                  # a trunk layer 16 wide
    _fb(q0=([14, 256, 256, 1], [RELU, RELU, TANH])),                 # a critic with a tanh output
    _fb(h1=_head(acts=RR), h2=_head(acts=RR)),                       # heads with a ReLU output
    _fb(post=([13, 256, 256, 2], RRN)),                              # a multiplier with two outputs
    _fb(q1=([14, 256, 256, 2], RRN)),                                # a critic with two outputs
    _fb(h1=_head(out=16), h2=_head(out=16), C=16),                   # C 16
    _fb(h1=_head(out=17), h2=_head(out=17), C=17),                   # C 17
    _fb(post=([12, 256, 256, 1], RRN)),                              # no post chain (its first din is cols0)
]
FB_WANT = [True, False, False, False, False, False, False, True, False, False, False, False, False, True, False,
           False]

# ---- the model fit: (S, A, trunk, diff head, log-var head)


def _ens(S=12, A=2, H=200, trunk=None, h1=None, h2=None):
    head = ([H, H, S + 1], SN)
    return (S, A, trunk or ([S + A, H, H], SS), h1 or head, h2 or head)


# bit 0: drpo_mlp_backward_ens (the NLL formed in the backward launch)
ENS_BWD = [
    _ens(),                                                          # the reference model, hidden 200
    _ens(H=256),                                                     # hidden 256
    _ens(H=128),                                                     # hidden 128
    _ens(S=63, A=1),                                                 # S + 1 = 64
    _ens(S=64, A=1),                                                 # S + 1 = 65
    _ens(h1=([200, 200, 13], [SWISH, TANH]), h2=([200, 200, 13], [SWISH, TANH])),   # a non-identity output
    _ens(h2=([200, 256, 13], SN)),                                   # unequal heads: hidden width
    _ens(h2=([200, 200, 13], [RELU, NONE])),                         # ... hidden activation
    _ens(h2=([200, 200, 12], SN)),                                   # ... output width
    _ens(h1=([200, 200, 200, 13], [SWISH, SWISH, NONE]), h2=([200, 200, 200, 13], [SWISH, SWISH, NONE])),  # depth 3
    _ens(trunk=([14, 257, 200], SS)),                                # a trunk layer 257 wide
    _ens(trunk=([14, 64, 200], [RELU, TANH])),                       # any trunk of admitted widths
]
ENS_BWD_WANT = [True, True, False, True, False, False, False, False, False, False, False, True]
# what drpo_mlp_backward_ens says when it refuses a case (after "drpo_mlp_backward_ens: ")
ENS_BWD_REFUSAL = {10: 'job 0: bad layer 0 of net 0'}
ENS_BWD_REFUSAL_DEFAULT = 'heads must be paired [H -> 200|256 -> S+1] (S+1 <= 64)'

# bit 1: drpo_ens_fit_fb (forward, NLL and backward-data in one launch)
ENS_FB = [
    _ens(),                                                          # the reference model, H 200
    _ens(H=256),                                                     # H 256
    _ens(H=128),                                                     # H 128
    _ens(A=52),                                                      # S + A = 64
    _ens(A=53),                                                      # S + A = 65
    _ens(S=15),                                                      # S + 1 = 16
    _ens(S=16),                                                      # S + 1 = 17
    _ens(trunk=([14, 200], [SWISH])),                                # trunk depth 1
    _ens(trunk=([14, 200, 200, 200], [SWISH] * 3)),                  # trunk depth 3
    _ens(trunk=([14, 200, 200], [RELU, SWISH])),                     # ReLU in place of swish: trunk layer 0
    _ens(trunk=([14, 200, 200], [SWISH, RELU])),                     # ... trunk layer 1
    _ens(h1=([200, 200, 13], [RELU, NONE]), h2=([200, 200, 13], [RELU, NONE])),   # ... the heads' hidden layers
    _ens(trunk=([14, 256, 200], SS)),                                # trunk layers of two widths
    _ens(h1=([200, 256, 13], SN), h2=([200, 256, 13], SN)),          # heads' hidden width not the trunk's
    _ens(h1=([200, 200, 13], [SWISH, TANH]), h2=([200, 200, 13], [SWISH, TANH])),   # a non-identity output
    _ens(h1=([200, 200, 200, 13], [SWISH, SWISH, NONE]), h2=([200, 200, 200, 13], [SWISH, SWISH, NONE])),  # depth 3
]
ENS_FB_WANT = [True, True, False, True, False, True, False, False, False, False, False, False, False, False, False,
               False]

# ---- rollout engine: (engine, recorded draws, eps_layout, H) -> the engine drpo_rollout runs
ROLLOUT = [
    ((0, False, 0, 10), 2),      # auto, device noise
    ((0, True, 0, 10), 1),       # recorded draws compacted per step
    ((0, True, 1, 10), 2),       # recorded draws by original row
    ((0, False, 0, 128), 2),     # the fused engine's longest horizon
    ((0, False, 0, 129), 1),
    ((0, True, 1, 129), 1),
    ((1, False, 0, 10), 1),      # explicit engines pass through
    ((2, False, 0, 10), 2),
    ((2, True, 0, 129), 2),
]
