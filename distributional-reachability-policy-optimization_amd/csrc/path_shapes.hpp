// The shape conditions of the fused paths, each written once. An entry point refuses what
// its kernel cannot run by calling these, and the exported path queries
// (include/drpo_hip.h "path queries", csrc/core.hip) are thin wrappers over the same
// functions, so a caller that picks its path and the entry point that admits it cannot
// drift apart. Plain functions over nl and the layers' din / dout / act: no pointer is
// read. Templated on the net type where drpo_mlp_net_t and drpo_mlp_bwd_net_t share a rule.
//
// A new fused path adds its condition here and its query to the ABI, never a predicate
// in the binding.
#pragma once
#include "common.hpp"

namespace drpo {

constexpr int MLP_MAXL = 3;   // layers of a net
constexpr int MLP_MAXN = 3;   // nets of a job

// 1..3 layers of 1..256 outputs, each reading the one before it, the first `din` columns
inline bool net_shape_ok(const drpo_mlp_net_t& n, int din) {
  if (n.nl < 1 || n.nl > MLP_MAXL) return false;
  for (int l = 0; l < n.nl; ++l) {
    if (n.L[l].din != din || n.L[l].dout < 1 || n.L[l].dout > 256) return false;
    din = n.L[l].dout;
  }
  return true;
}

template <class NetA, class NetB>
inline bool same_layers(const NetA& a, const NetB& b) {
  if (a.nl != b.nl) return false;
  for (int l = 0; l < a.nl; ++l)
    if (a.L[l].din != b.L[l].din || a.L[l].dout != b.L[l].dout || a.L[l].act != b.L[l].act) return false;
  return true;
}

// A pair job (the kernel's pair_nets assumptions; the kernel trusts the checked `pair`
// flag): two 3-layer ReLU nets of one shape [K <= 16 or 49..64 -> 256 -> 256 -> <= 16].
inline bool pair_shapes(const drpo_mlp_net_t& A, const drpo_mlp_net_t& B) {
  if (A.nl != 3 || !same_layers(A, B)) return false;
  const int k0 = (A.L[0].din + 15) >> 4;
  return (k0 == 1 || k0 == 4) && A.L[0].dout == 256 && A.L[1].din == 256 && A.L[1].dout == 256 &&
         A.L[2].dout <= 16 && A.L[0].act == ACT_RELU && A.L[1].act == ACT_RELU && A.L[2].act == ACT_NONE;
}

// Trunk-mode job whose two heads are [256 -> N, act0] -> [N -> n<=16, act1] each (the
// constraint critic's mean and log-std heads, src/ssac.py:46-92): both heads' hidden
// layers run as ONE paired layer over the trunk output (2N output columns, one
// k-loop) and both output layers as one split-K narrow pair, so the job's serial
// chain is 4 layers instead of 6.
// (host: the ccb_out check of drpo_mlp_forward_multi)
__host__ __device__ __forceinline__ bool heads_pairable(const drpo_mlp_fwd_t* __restrict__ a) {
  if (a->nnets != 3) return false;
  const drpo_mlp_net_t& n1 = a->net[1];
  const drpo_mlp_net_t& n2 = a->net[2];
  return n1.nl == 2 && n2.nl == 2 && n1.L[0].din == 256 && n2.L[0].din == 256 && n1.L[0].dout == n2.L[0].dout &&
         n1.L[0].act == n2.L[0].act && n1.L[1].act == n2.L[1].act && n1.L[1].dout <= 16 && n2.L[1].dout <= 16;
}

// The post chain of a job with the constraint bound: a net on [src[0] (<= 63 columns), bound].
inline bool post_shapes(int cols0, const drpo_mlp_net_t& post) {
  return cols0 + 1 <= 64 && net_shape_ok(post, cols0 + 1);
}

// Two heads of the same shape on a shared trunk (the dynamics model's diff / log-var
// heads, src/dynamics.py:84-91; the constraint critic's mean / log-std heads,
// src/ssac.py:46-92), each [trunk width -> H -> out] with an identity output layer:
// backed through TOGETHER. Their output layers' products run side by side (one
// two-input pair layer), and the trunk-output gradient -- the sum of the two heads'
// hidden-layer products -- is ONE product with the concatenated K (dZ_1 | dZ_2) x
// [W_1; W_2]: three dependent GEMM phases instead of five, and no LDS accumulation.
// (host: drpo_mlp_backward_ens checks its heads with it)
__host__ __device__ __forceinline__ bool bwd_paired_heads(const drpo_mlp_bwd_t& a) {
  if (!a.trunk || a.split_heads || a.nnets != 3) return false;
  const drpo_mlp_bwd_net_t &h1 = a.net[1], &h2 = a.net[2];
  if (h1.nl != 2 || h2.nl != 2 || h1.dx || h2.dx) return false;
  for (int l = 0; l < 2; ++l)
    if (h1.L[l].din != h2.L[l].din || h1.L[l].dout != h2.L[l].dout || h1.L[l].act != h2.L[l].act) return false;
  const int hid = h1.L[0].dout, out = h1.L[1].dout;
  return h1.L[1].act == ACT_NONE && (hid == 200 || hid == 256) && out <= 64 && h1.L[0].din <= 256;
}

// what every backward launch requires of a layer's widths
inline bool bwd_layer_dims(const drpo_mlp_bwd_layer_t& L) {
  return L.din >= 1 && L.din <= 256 && L.dout >= 1 && L.dout <= 256;
}

// drpo_mlp_backward_ens: the NLL upstream assumes the paired head shape [H -> 200|256 ->
// S+1] (S+1 <= 64), also when each head then runs in a workgroup of its own (split_heads)
inline bool ens_bwd_shapes(const drpo_mlp_bwd_t& a, int S1) {
  drpo_mlp_bwd_t shape = a;
  shape.split_heads = 0;
  return bwd_paired_heads(shape) && a.net[1].L[1].dout == S1;
}

// drpo_ens_fit_fb: the ensemble trunk [S+A <= 64 -> H -> H] and two heads [H -> H -> S+1 <= 16]
// (swish hidden layers, identity outputs, H = 200 | 256), the backward describing the same layers
inline bool ens_fit_fb_shapes(const drpo_mlp_fwd_t& f, const drpo_mlp_bwd_t& bd, int S) {
  const drpo_mlp_net_t &tr = f.net[0], &h1 = f.net[1], &h2 = f.net[2];
  const int S1 = S + 1;
  const int din0 = f.cols[0] + f.cols[1];
  const int H = tr.nl == 2 ? tr.L[1].dout : -1;
  bool ok = f.trunk && f.nnets == 3 && tr.nl == 2 && h1.nl == 2 && h2.nl == 2 && f.cols[2] == 0 && f.cols[0] == S &&
            din0 >= 1 && din0 <= 64 && (H == 200 || H == 256) && tr.L[0].dout == H && tr.L[0].din == din0 &&
            tr.L[1].din == H && S1 <= 16 && bd.trunk && bd.nnets == 3;
  for (const drpo_mlp_net_t* n : {&h1, &h2})
    ok = ok && n->L[0].din == H && n->L[0].dout == H && n->L[1].din == H && n->L[1].dout == S1 &&
         n->L[0].act == ACT_SILU && n->L[1].act == ACT_NONE;
  ok = ok && tr.L[0].act == ACT_SILU && tr.L[1].act == ACT_SILU;
  for (int j = 0; j < 3; ++j)
    for (int l = 0; l < 2; ++l)
      ok = ok && bd.net[j].L[l].din == f.net[j].L[l].din && bd.net[j].L[l].dout == f.net[j].L[l].dout;
  return ok;
}

// drpo_mlp_fb_multi, a layer of a job's last forward and backward: hidden layers (every
// layer of a trunk, all but the last of any other net) are ReLU and wider than 16 (their
// masks stay on chip), outputs identity
template <class Layer>
inline bool fb_layer_shape(const Layer& L, bool hidden) {
  return L.act == (hidden ? ACT_RELU : ACT_NONE) && (!hidden || L.dout > 16);
}
template <class Net>
inline bool fb_net_shapes(const Net& n, bool trunk) {
  for (int l = 0; l < n.nl; ++l)
    if (!fb_layer_shape(n.L[l], trunk || l < n.nl - 1)) return false;
  return true;
}
// ... its single-net job: one output (the -1/B upstream)
template <class Net>
inline bool fb_single_shapes(const Net& n) {
  return n.L[n.nl - 1].dout == 1;
}
// ... its trunk job: the constraint-critic upstream on paired 256-wide heads [256 -> 256 -> C]
inline bool fb_trunk_shapes(const drpo_mlp_fwd_t* f, const drpo_mlp_bwd_t& b, int C) {
  return heads_pairable(f) && bwd_paired_heads(b) && b.net[1].L[0].dout == 256 &&
         b.net[0].L[b.net[0].nl - 1].dout == 256 && b.net[1].L[1].dout == C;
}
// ... the post chain of a job's first forward: one output (the multiplier)
inline bool fb_post_shapes(const drpo_mlp_net_t& post) { return post.nl > 0 && post.L[post.nl - 1].dout == 1; }

// the engine drpo_rollout runs: compacted recorded draws and horizons beyond the fused
// engine's need the step engine
inline int rollout_engine(const drpo_rollout_desc_t* d) {
  if (d->engine != 0) return d->engine;
  return (d->eps_a && d->eps_layout == 0) || d->H > DRPO_ROLLOUT_FUSED_MAX_H ? 1 : 2;
}

// drpo_rollout_adjoint: the ensemble's trunk [S+A <= 64 -> H -> H] and diff head [H -> H -> S+1 <= 16]
// (the widths drpo_ens_fit_fb takes: H = 200 | 256, swish)
inline bool rollout_adjoint_shapes(int S, int A, int Hm) {
  return S >= 1 && A >= 1 && S + A <= 64 && S + 1 <= 16 && (Hm == 200 || Hm == 256);
}

}  // namespace drpo
