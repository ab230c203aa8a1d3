// The body of the two 256-thread passes of the two-half backward (described in fused_bwd.h, which includes this under
// FBH_CTX = 0 for bwd_dz_wgrs64_kernel, the first half, and under FBH_CTX = 1 for bwd_dctx_wgctx64_kernel, the context
// pass): the scaffold and, under `if constexpr (CTX)`, the two policies' sections, each marked [policy].  Not a header
// of its own: it opens at the brace behind a kernel's parameter list and reads that kernel's names -- a, chunks_per_b,
// chunk_t, bias_part, part.  Both passes stage a tile of 128 "A" rows and two tiles of 64 rows (Ta, Tb) per 64 time
// steps, form the transposed product W^T A with W in registers and the weight gradient A Ta'^T, and write one tile:
//                       A rows          Ta        Tb                    W            written
//   first half          dxo | dskip     tanh      sigmoid               Wr | Ws      df | dg   (As, 128 rows)
//   context pass        df | dg         context   dctx so far, updated  Wcf | Wcg    dctx      (Tb, 64 rows)
{
  // [policy] the two 64-row tiles under each kernel's own names (the names decide the tiles' order in LDS, and with it
  // the kernels' instructions): tanh | sigmoid, or the context | dctx
#if FBH_CTX
#define Ta Cx
#define Tb Dc
#else
#define Ta Th
#define Tb Sg
#endif
  constexpr bool CTX = FBH_CTX != 0;
  // The kernels are no templates, so both policies' sections are compiled in both: each reads its own arguments
  // through az / ac, and the kernel that is not its own gives it a zeroed stand-in, which nothing executed reads.
#if FBH_CTX
  const FusedBwdCArgs &ac = a;
  const FusedBwdAArgs az = {};
#else
  const FusedBwdAArgs &az = a;
  const FusedBwdCArgs ac = {};
#endif
  constexpr int C = FB_C, LD = W2_LD, TT = W2_T;
  __shared__ __attribute__((aligned(16))) float As[2 * C][LD];  // the A rows; in the first half later df | dg
  __shared__ __attribute__((aligned(16))) float Ta[C][LD];
  __shared__ __attribute__((aligned(16))) float Tb[C][LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / chunks_per_b, ch = blockIdx.x - b * chunks_per_b;
  const int li = lane & 31, lh = lane >> 5, h4 = 4 * lh;
  const int tb = (a.t_begin & ~TILE_ALIGN) + ch * chunk_t, te = min(a.t_end, tb + chunk_t);
  // [policy] first half: dskip starts at t_skip0; the last layer has no dxo (its residual output is unused)
  const int skip_lo = max(a.t_begin, az.t_skip0);
  const bool has_dxo = az.dxo.p != nullptr;

  // ---- B operand of the transposed product: W[o][32 wc + li] for o = 2 kk + lh, in registers
  const int wt = wave >> 1, wc = wave & 1;  // block: t in [32 wt, +32), c in [32 wc, +32)
  float wreg[C];
#pragma unroll
  for (int kk = 0; kk < C; ++kk) {
    const int o = 2 * kk + lh;
    if constexpr (CTX)  // [policy]
      wreg[kk] = o < C ? ac.wcf[(size_t)o * C + 32 * wc + li] : ac.wcg[(size_t)(o - C) * C + 32 * wc + li];
    else
      wreg[kk] = o < C ? (has_dxo ? az.wr[(size_t)o * C + 32 * wc + li] : 0.f)
                       : az.ws[(size_t)(o - C) * C + 32 * wc + li];
  }
  // weight-gradient block of this wave (as wgrad2_kernel<.., 1>): rows [64 wm, +64), cols [32 wn, +32)
  const int wm = wave >> 1, wn = wave & 1;
  f32x16 accw[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[i][r] = 0.f;

  // ---- staging: thread -> rows (tid >> 4) + 16 p, columns 4 (tid & 15) .. +3
  const int srow = tid >> 4, st = 4 * (tid & 15);
  f4 areg[8], tareg[4], tbreg[4];
  float bsum[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) bsum[p] = 0.f;
  unsigned azero = 0;  // [policy] first half: the A row blocks to zero at the LDS store
  // [policy] the tensors behind the A rows (dxo | dskip, or dfg), behind Ta and Tb, and the one written
  const Act &ta_t = CTX ? ac.ctx : az.th, &tb_t = CTX ? ac.dctx : az.sg, &out_t = CTX ? ac.dctx : az.dfg;
  const __amdgpu_buffer_rsrc_t dxob = fb_rsrc(az.dxo.p + (size_t)b * az.dxo.sb);
  const __amdgpu_buffer_rsrc_t dskb = fb_rsrc(az.dskip.p + (size_t)b * az.dskip.sb);
  const __amdgpu_buffer_rsrc_t dfab = fb_rsrc(ac.dfg.p + (size_t)b * ac.dfg.sb);
  const __amdgpu_buffer_rsrc_t tab = fb_rsrc(ta_t.p + (size_t)b * ta_t.sb);
  const __amdgpu_buffer_rsrc_t tbb = fb_rsrc(tb_t.p + (size_t)b * tb_t.sb);
  const __amdgpu_buffer_rsrc_t outb = fb_rsrc(out_t.p + (size_t)b * out_t.sb);
  const int vo_dxo = 4 * (srow * az.dxo.ld + st), vo_dsk = 4 * (srow * az.dskip.ld + st), vo_dfa = 4 * (srow * ac.dfg.ld + st);
  const int vo_ta = 4 * (srow * ta_t.ld + st), vo_tb = 4 * (srow * tb_t.ld + st), vo_out = 4 * (srow * out_t.ld + st);
  auto gload = [&](int t0) {
    int srow_q = srow;
    asm volatile("" : "+v"(srow_q));  // (the edge path's row addresses are formed behind this, not kept across the loop)
    const int t = t0 + st;
    // [policy] interior: the tile lies inside every live row's range (one test per tile, workgroup-uniform).  First
    // half: rows whose range misses the tile altogether (dskip before t_skip0, the absent dxo of the last layer) load
    // a row that IS valid and are zeroed at the LDS store.  Context pass: one validity range.
    bool interior = t0 >= a.t_begin && t0 + TT <= te;
    if constexpr (!CTX) {
      const bool s_full = t0 >= skip_lo && t0 + TT <= te, s_none = t0 + TT <= skip_lo;
      azero = (has_dxo ? 0u : 0x0Fu) | (s_none ? 0xF0u : 0u);
      interior = interior && (s_full || s_none);
    }
    if (interior) {
      // raw buffer loads (fb_load16): per-lane offset of (row srow, column st) + scalar offset of the row block and the
      // tile, sixteen back-to-back 16-byte loads (the row-block offsets formed here, behind a fence, not hoisted)
      // [policy] the A rows: dxo | dskip with the row blocks of `azero` taken from a valid row, or dfg
      int ld_dxo = 4 * az.dxo.ld, ld_dsk = 4 * az.dskip.ld, ld_dfa = 4 * ac.dfg.ld, ld_ta = 4 * ta_t.ld, ld_tb = 4 * tb_t.ld;
      if constexpr (CTX)
        asm volatile("" : "+s"(ld_dfa), "+s"(ld_ta), "+s"(ld_tb));
      else
        asm volatile("" : "+s"(ld_dxo), "+s"(ld_dsk), "+s"(ld_ta), "+s"(ld_tb));
      const int c4 = 4 * t0;
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        if constexpr (CTX)
          areg[p] = fb_load16(dfab, vo_dfa, 16 * p * ld_dfa + c4);
        else if ((azero >> p) & 1u)
          areg[p] = fb_load16(tab, vo_ta, c4);
        else if (p < 4)
          areg[p] = fb_load16(dxob, vo_dxo, 16 * p * ld_dxo + c4);
        else
          areg[p] = fb_load16(dskb, vo_dsk, 16 * (p - 4) * ld_dsk + c4 - 4 * az.t_base);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        tareg[p] = fb_load16(tab, vo_ta, 16 * p * ld_ta + c4);
        tbreg[p] = fb_load16(tbb, vo_tb, 16 * p * ld_tb + c4);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int p = 0; p < 8; ++p) {  // [policy]
        if constexpr (CTX)
          areg[p] = ld4_edge(ac.dfg.at(b, 16 * p + srow_q, 0), t, a.t_begin, te);
        else if (p < 4)
          areg[p] = has_dxo ? ld4_edge(az.dxo.at(b, 16 * p + srow_q, 0), t, a.t_begin, te) : kZero4;
        else
          areg[p] = ld4_edge(az.dskip.at(b, 16 * (p - 4) + srow_q, 0) - az.t_base, t, skip_lo, te);
      }
      azero = 0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        tareg[p] = ld4_edge(ta_t.at(b, 16 * p + srow_q, 0), t, a.t_begin, te);
        tbreg[p] = ld4_edge(tb_t.at(b, 16 * p + srow_q, 0), t, a.t_begin, te);
      }
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      if constexpr (!CTX)  // [policy]
        if ((azero >> p) & 1u) areg[p] = kZero4;
      *(f4 *)&As[16 * p + srow][st] = areg[p];
      bsum[p] += (areg[p].x + areg[p].y) + (areg[p].z + areg[p].w);  // bias gradient = row sums
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *(f4 *)&Ta[16 * p + srow][st] = tareg[p];
      *(f4 *)&Tb[16 * p + srow][st] = tbreg[p];
    }
  };

  gload(tb);
  lstore();
  __syncthreads();
  for (int t0 = tb; t0 < te; t0 += TT) {
    const bool more = t0 + TT < te;
    if (more) gload(t0 + TT);  // the next tile's loads fly under this tile's MFMAs
    __builtin_amdgcn_sched_barrier(0);
    // ---- the transposed product (32 t x 32 c) = sum over the 128 rows of the tile
    f32x16 accd;
#pragma unroll
    for (int r = 0; r < 16; ++r) accd[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < C; ++kk)
      accd = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * kk + lh][32 * wt + li], wreg[kk], accd, 0, 0, 0);
    // ---- weight gradient: (64 x 32) += A (64 x 64 t) Ta'^T
    if constexpr (CTX) {
      // [policy] Ta' = the context, on the bf16 matrix cores as in the second half (bf16 x 3)
#pragma unroll
      for (int G = 0; G < TT / 16; ++G) {
        u32x4 ah[2], am[2], al[2], ch, cm, cl;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const f4 v0 = *(const f4 *)&As[64 * wm + 32 * mi + li][16 * G + 2 * h4];
          const f4 v1 = *(const f4 *)&As[64 * wm + 32 * mi + li][16 * G + 2 * h4 + 4];
          const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
          bf3_split8(v, ah[mi], am[mi], al[mi]);
        }
        {
          const f4 v0 = *(const f4 *)&Ta[32 * wn + li][16 * G + 2 * h4], v1 = *(const f4 *)&Ta[32 * wn + li][16 * G + 2 * h4 + 4];
          const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
          bf3_split8(v, ch, cm, cl);
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) bf3_mfma6r(accw[mi], ah[mi], am[mi], al[mi], ch, cm, cl);
      }
    } else {
      // [policy] Ta' = z = tanh sigmoid, formed on the fly, as wgrad2_kernel does it (four k-steps per ds_read_b128).
      // (r3, measured: this product on the bf16 matrix cores as in the second half -- 115.9 against 100.4 us: the
      // planes do not fit beside this kernel's 248 registers, 13 spill in the tile loop.  It stays on fp32 MFMAs.)
      // (... and the dz product above with its K split between wave pairs as in the second half's dx: 111.3 against
      // 104.9 us -- this kernel is bound by its barriers and its bytes, a third barrier per tile costs more than the
      // matrix time it saves.)
#pragma unroll
      for (int g = 0; g < TT / 8; ++g) {
        f4 av[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) av[mi] = *(const f4 *)&As[64 * wm + 32 * mi + li][8 * g + h4];
        const f4 tv = *(const f4 *)&Ta[32 * wn + li][8 * g + h4], sv = *(const f4 *)&Tb[32 * wn + li][8 * g + h4];
        const f4 zv = f4{tv.x * sv.x, tv.y * sv.y, tv.z * sv.z, tv.w * sv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
            accw[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4_get(av[mi], j), f4_get(zv, j), accw[mi], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // [policy] what becomes of the product.  This lane holds it for channel 32 wc + li at t = 32 wt + 8 q + 4 lh + e.
    // Both policies wait for the next tile's loads HERE, in front of the barrier that precedes the stores: the loads
    // have had the whole MFMA section to land.  On gfx9 stores count in vmcnt too, and the number of stores below
    // depends on the path (edge tiles), so the compiler's own wait in front of lstore() was vmcnt(0) -- behind this
    // tile's global stores, i.e. one full store round trip per tile with the matrix cores idle.
    if constexpr (CTX) {
      // added to the dctx tile in LDS by the lane that owns the element (no staging copy of the product: two barriers
      // per tile, not three)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int tc = 32 * wt + 8 * q + h4;
        const f4 o = *(const f4 *)&Tb[32 * wc + li][tc];
        *(f4 *)&Tb[32 * wc + li][tc] =
            f4{o.x + accd[4 * q], o.y + accd[4 * q + 1], o.z + accd[4 * q + 2], o.w + accd[4 * q + 3]};
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
      __syncthreads();  // the dctx tile is complete AND every wave has read As / Ta
      FB_TILE_STORE(4, 16, out_t, outb, vo_out, a.t_begin, *(const f4 *)&Tb[16 * p + srow][st], Tb[16 * p + srow][st + e]);
      // (no barrier here: a thread's lstore() overwrites exactly the Tb elements the same thread has just read for its
      // global stores; As / Ta were last read before the barrier above)
    } else {
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
      __syncthreads();  // every wave has read the tile: As becomes the df | dg staging tile
      // the gate derivative (after the barrier, straight into the staging tile: held in registers across it, the 32
      // values spilled next to the next tile's 64 staging registers.  Stored to global memory straight from this
      // layout -- 16 bytes per lane and row, no staging tile, two barriers per tile instead of three -- the kernel took
      // 104.6 against 98.8 us: the write path wants whole cache lines.)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int tc = 32 * wt + 8 * q + h4;
        const f4 tv = *(const f4 *)&Ta[32 * wc + li][tc], sv = *(const f4 *)&Tb[32 * wc + li][tc];
        const f4 dz = f4{accd[4 * q], accd[4 * q + 1], accd[4 * q + 2], accd[4 * q + 3]};
        *(f4 *)&As[32 * wc + li][tc] =
            f4{dz.x * sv.x * (1.0f - tv.x * tv.x), dz.y * sv.y * (1.0f - tv.y * tv.y),
               dz.z * sv.z * (1.0f - tv.z * tv.z), dz.w * sv.w * (1.0f - tv.w * tv.w)};
        *(f4 *)&As[C + 32 * wc + li][tc] =
            f4{dz.x * tv.x * sv.x * (1.0f - sv.x), dz.y * tv.y * sv.y * (1.0f - sv.y),
               dz.z * tv.z * sv.z * (1.0f - sv.z), dz.w * tv.w * sv.w * (1.0f - sv.w)};
      }
      __syncthreads();
      FB_TILE_STORE(8, 16, out_t, outb, vo_out, a.t_begin, *(const f4 *)&As[16 * p + srow][st], As[16 * p + srow][st + e]);
      // (no barrier here: a thread's lstore() overwrites exactly the staging elements the same thread has just read for
      // its global stores, and Ta / Tb were last read before the barrier above)
    }
    if (more) {
      lstore();
      __syncthreads();
    }
  }
  // ---- this workgroup's slab and bias partial sums (wgrad2_kernel's format, m_rows_pad 128, n_cols_pad 64)
  FB_SLAB_STORE(accw, 64 * wm, 32, 32 * wn, 0, 64, lane);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    float v = bsum[p];  // 16 lanes share a row
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    if ((tid & 15) == 0) bias_part[(size_t)blockIdx.x * 128 + 16 * p + srow] = v;
  }
}
#undef Ta
#undef Tb
