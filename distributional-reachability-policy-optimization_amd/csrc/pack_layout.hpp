// The packed weight mirrors' layout: the one statement of it.
//
// drpo_pack_weights (pack.hip) rewrites PyTorch-layout weights W [nbatch][dout][din]
// (nn.Linear / BatchedLinear, src/torch_util.py:190-211, src/dynamics.py:26-52) into the
// fragment-linear layouts the MFMA tile streams (tile_dense in common.hpp). A fragment is
// 16 x 16 elements = 64 lanes x 4 components = 256 floats:
//   P  (forward,  y = x W^T):  P [(cb*NKS + s)*256 + 4*l + i] = W[16cb + (l&15)][16s + 4(l>>4) + i]
//   PT (backward, dx = dz W):  PT[(cb*NCB + s)*256 + 4*l + i] = W[16s + 4(l>>4) + i][16cb + (l&15)]
// with NKS = pack_frags(din), NCB = pack_frags(dout) and zero padding outside
// [dout) x [din). PT is the forward mirror of W^T, so both mirrors of a matrix have
// pack_matrix_floats(din, dout) floats, and member z of a [nbatch][dout][din] weight
// starts that many floats times z after member 0 (pack_member_base).
//
// pack_kernel walks the map from the fragment side (lane -> its 4 elements); the optimizer
// and the weight-gradient launch's fused step refresh single elements or aligned runs of 4
// (one lane's float4) and use the index functions below.
#pragma once
#include <stdint.h>

namespace drpo {

constexpr int PACK_FRAG_FLOATS = 256;

// 16-wide fragments covering n outputs or inputs
__host__ __device__ constexpr int pack_frags(int n) { return (n + 15) >> 4; }

// floats of one mirror of one [dout][din] matrix (== drpo_packed_size)
__host__ __device__ constexpr int64_t pack_matrix_floats(int din, int dout) {
  return (int64_t)pack_frags(dout) * pack_frags(din) * PACK_FRAG_FLOATS;
}

// first float of member z of a matrix whose member 0 starts at poff (drpo_pack_map_t.poff)
__host__ __device__ constexpr int64_t pack_member_base(int64_t poff, int z, int ncb, int nks) {
  return poff + (int64_t)z * ncb * nks * PACK_FRAG_FLOATS;
}

// Forward mirror: W[o][k] is component k&3 of lane ((k>>2)&3)*16 + (o&15) of fragment
// (o>>4, k>>4); nks = pack_frags(din). For k % 4 == 0 this is component 0 of the float4
// holding W[o][k .. k+3].
__host__ __device__ constexpr int64_t pack_fwd_index(int o, int k, int nks) {
  return ((int64_t)((o >> 4) * nks + (k >> 4)) << 8) + ((((k >> 2) & 3) * 16 + (o & 15)) << 2) + (k & 3);
}

// Transposed mirror (the forward mirror of W^T): W[o][k] is component o&3 of lane
// ((o>>2)&3)*16 + (k&15) of fragment (k>>4, o>>4); ncb = pack_frags(dout). For o % 4 == 0
// this is component 0 of the float4 holding W[o .. o+3][k].
__host__ __device__ constexpr int64_t pack_tr_index(int o, int k, int ncb) { return pack_fwd_index(k, o, ncb); }

}  // namespace drpo
