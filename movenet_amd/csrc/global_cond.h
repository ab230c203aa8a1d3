// Global conditioning on a class label: the small kernels around the layer kernels.
//
// A label's vector e_b (C floats per sequence) enters every gated layer where local context does, as a column that is
// constant in time:  f_l += Wcf_l e_b + bcf_l,  g_l += Wcg_l e_b + bcg_l.
//   general path: context_add_global_kernel adds e_b to (or fills with it) every time row of the generators' time-major
//                 context copy; the conditioned kernels then run as they are.
//   fast path (C = K = 64, no video): the term is ONE 2C-vector per (layer, sequence).  fp32:
//     forward   global_bias_kernel            gb[l][b] = [Wcf_l e_b + bcf_l | Wcg_l e_b + bcg_l], all layers in one launch;
//                                             fused_layer64s_bf3_kernel<true> adds it in front of tanh / sigmoid
//     backward  global_rowsum_kernel          r[l][b] = sum over the layer's valid columns of (df | dg)(b, :, t), read from
//                                             the dfg tensor bwd_layer64_kernel<true> writes (choice (b) of the two the
//                                             design names: nothing inside the 220-register layer kernel changes, at the
//                                             price of one write and one read of (B, 2C, T) floats per layer)
//               global_bias_backward_kernel   dWcf_l = sum_b r_f (x) e_b, dbcf_l = sum_b r_f (same for the gate),
//                                             de_b = sum_l Wcf_l^T r_f + Wcg_l^T r_g
//   bf16 (fused_bf16.h, the GLOBAL instantiations; choice (a)): the same global_bias_kernel and
//   global_bias_backward_kernel around layer kernels that start f | g from gb and sum the rows of df | dg themselves;
//               global_rowsum_reduce_kernel   r[l][b] = sum over the layer kernel's workgroups of their partial row sums
// Every sum runs in a fixed order (the backward's in double): no atomics, the same bits run to run.
#pragma once

#include "common.h"

namespace mvn {

// ctx_tm (batch, t_len, C) time-major: every time row of sequence b (+)= glob[b][0:C]
__global__ __launch_bounds__(256) void context_add_global_kernel(float *__restrict__ ctx_tm, const float *__restrict__ glob,
                                                                 int C, long long per_seq, int fill) {
  const int b = blockIdx.y;
  float *row = ctx_tm + (size_t)b * per_seq;
  const float *gv = glob + (size_t)b * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per_seq; i += (long long)gridDim.x * 256) {
    const float v = gv[(int)(i % C)];
    row[i] = fill ? v : row[i] + v;
  }
}

constexpr int GC_LAYERS = 32;  // layers per launch (pointer tables travel as kernel arguments)
struct GlobalCondArgs {
  const float *wcf[GC_LAYERS], *wcg[GC_LAYERS], *bcf[GC_LAYERS], *bcg[GC_LAYERS];
};
struct GlobalCondGrads {
  float *dwcf[GC_LAYERS], *dwcg[GC_LAYERS], *dbcf[GC_LAYERS], *dbcg[GC_LAYERS];
};

// grid (batch, layers of this launch), 128 threads: row j < 64 of the filter, j >= 64 of the gate.  C = 64.
__global__ __launch_bounds__(128) void global_bias_kernel(GlobalCondArgs p, const float *__restrict__ e, float *__restrict__ gb,
                                                          int batch) {
  __shared__ float ev[64];
  const int b = blockIdx.x, l = blockIdx.y, j = threadIdx.x;
  if (j < 64) ev[j] = e[(size_t)b * 64 + j];
  __syncthreads();
  const int row = j & 63;
  const float *w = (j < 64 ? p.wcf[l] : p.wcg[l]) + row * 64;
  float acc = 0.f;
#pragma unroll 16
  for (int c = 0; c < 64; ++c) acc = __builtin_fmaf(w[c], ev[c], acc);
  gb[((size_t)l * batch + b) * 128 + j] = acc + (j < 64 ? p.bcf[l] : p.bcg[l])[row];
}

// grid (32, batch), 256 threads: one wave per row of the (2C = 128, Tp) df | dg tensor of one sequence, columns
// [t_lo, t_end) (what the layer kernel wrote; the rest of a row is stale).  r: (batch, 128) of this layer.
__global__ __launch_bounds__(256) void global_rowsum_kernel(const float *__restrict__ dfg, long long sb, int ld, int t_lo,
                                                            int t_end, float *__restrict__ r) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const float *src = dfg + (size_t)b * sb + (size_t)row * ld;
  // (double: a row of a 16000-step clip is 250 addends per lane of mixed sign, and the sum feeds three gradients; the
  // kernel waits for memory either way)
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int t = t_lo + lane;
  for (; t + 192 < t_end; t += 256) {
    s0 += src[t];
    s1 += src[t + 64];
    s2 += src[t + 128];
    s3 += src[t + 192];
  }
  for (; t < t_end; t += 64) s0 += src[t];
  double v = (s0 + s1) + (s2 + s3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) r[(size_t)b * 128 + row] = (float)v;
}

// The bf16 layer backward's row sums (fused_bf16.h: bwd_layer64_bf16_kernel<true> sums df | dg inside the kernel, one
// 128-float partial per workgroup, workgroup = sequence b x chunk ch): r[b][row] = sum_ch g_part[b chunks + ch][row], in
// double and in chunk order.  grid (batch), 128 threads.
__global__ __launch_bounds__(128) void global_rowsum_reduce_kernel(const float *__restrict__ g_part, int chunks,
                                                                   float *__restrict__ r) {
  const int b = blockIdx.x, row = threadIdx.x;
  double acc = 0.0;
  for (int ch = 0; ch < chunks; ++ch) acc += (double)g_part[((size_t)b * chunks + ch) * 128 + row];
  r[(size_t)b * 128 + row] = (float)acc;
}

// grid (layers of this launch + batch), 256 threads.  r: (layers, batch, 128) from this launch's first layer on.
//   blocks [0, n_layers): the layer's dWcf | dWcg (64 x 64 each) and dbcf | dbcg, written (the slots are this path's own)
//   blocks [n_layers, n_layers + batch): de_b over the launch's layers; `accumulate` adds to what an earlier launch left
__global__ __launch_bounds__(256) void global_bias_backward_kernel(GlobalCondArgs p, GlobalCondGrads g, const float *__restrict__ r,
                                                                   const float *__restrict__ e, float *__restrict__ de,
                                                                   int n_layers, int batch, int accumulate) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < n_layers) {
    const int l = blockIdx.x;
    const float *rl = r + (size_t)l * batch * 128;
    for (int i = tid; i < 2 * 64 * 64; i += 256) {
      const int gate = i >> 12, j = (i >> 6) & 63, c = i & 63;
      double acc = 0.0;
      for (int b = 0; b < batch; ++b) acc += (double)rl[(size_t)b * 128 + 64 * gate + j] * (double)e[(size_t)b * 64 + c];
      (gate ? g.dwcg[l] : g.dwcf[l])[j * 64 + c] = (float)acc;
    }
    if (tid < 128) {
      double acc = 0.0;
      for (int b = 0; b < batch; ++b) acc += (double)rl[(size_t)b * 128 + tid];
      (tid < 64 ? g.dbcf[l] : g.dbcg[l])[tid & 63] = (float)acc;
    }
    return;
  }
  __shared__ double part[4][64];
  const int b = blockIdx.x - n_layers, c = tid & 63, q = tid >> 6;  // wave q takes rows 32 q .. 32 q + 31 of f | g
  double acc = 0.0;
  for (int l = 0; l < n_layers; ++l) {
    const float *rv = r + ((size_t)l * batch + b) * 128 + 32 * q;
    const float *w = (q < 2 ? p.wcf[l] : p.wcg[l]) + (32 * (q & 1)) * 64 + c;
    for (int j = 0; j < 32; ++j) acc += (double)w[j * 64] * (double)rv[j];
  }
  part[q][c] = acc;
  __syncthreads();
  if (q == 0) {
    const double v = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
    de[(size_t)b * 64 + c] = (float)(accumulate ? (double)de[(size_t)b * 64 + c] + v : v);
  }
}

}  // namespace mvn
