// The body of both layer backward kernels: the scaffold and, under `if constexpr (BF3)`, the two operand policies'
// sections (described in fused_bwd_l.h, which includes this under FBL_BF3 = 1 for bwd_layer64_kernel; fused_bf16.h
// includes it under FBL_BF3 = 0 for bwd_layer64_bf16_kernel).  Not a header of its own: it opens at the brace behind a
// kernel's parameter list and reads that kernel's names -- a, chunks_per_b, chunk_t, rs_bias_part, rs_part, fg_part and
// the template parameter WRITE_DFG; under FBL_BF3 = 0 also GLOBAL and g_part, which the fp32 kernel does not have.
{
  constexpr bool BF3 = FBL_BF3 != 0;
#if FBL_BF3
  constexpr bool GLOBAL = false;  // (no fp32 form: its label's row sums come from the dfg output, global_cond.h)
  float *const g_part = nullptr;
#endif
  static_assert(!(GLOBAL && WRITE_DFG), "the label's row sums and the dfg output are separate kernels");
  constexpr int C = FB_C, LD = W2_LD, TT = W2_T;
  extern __shared__ __attribute__((aligned(16))) float fbl_lds[];
  float (*U)[LD] = (float (*)[LD])fbl_lds;                      // [dxo; dskip], then [x(t - d); x(t)]
  float (*Gt)[LD] = (float (*)[LD])(fbl_lds + FBL_TILE_F);      // tanh | sigmoid, then df | dg
  float (*O)[LD] = (float (*)[LD])(fbl_lds + 2 * FBL_TILE_F);   // dxo -> A' | P0
  unsigned short *wimg = (unsigned short *)(fbl_lds + 3 * FBL_TILE_F);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / chunks_per_b, ch = blockIdx.x - b * chunks_per_b;
  const int li = lane & 31, lh = lane >> 5, h4 = 4 * lh;
  const int tb = (a.t_lo & ~TILE_ALIGN) + ch * chunk_t, te = min(a.t_end, tb + chunk_t);
  const int skip_lo = max(a.t_lo, a.t_skip0);
  const bool has_dxo = a.ga.p != nullptr;
  // timing builds (wrong results; python -m movenet_amd.csrc.build --stamps --exp=N): 71 no global loads after a
  // workgroup's first tile, 72 no global stores, 73 both, 74 no MFMAs -- BF3 only
#if MVN_EXP == 71 || MVN_EXP == 73
  const bool ld_ok = !BF3 || a.t_end < 0;  // (never: the loads stay in the code, none is executed)
#else
  constexpr bool ld_ok = true;
#endif
#if MVN_EXP == 72 || MVN_EXP == 73
  const bool st_ok = !BF3 || a.t_end < 0;
#else
  constexpr bool st_ok = true;
#endif

  // ---- [Wr | Ws]^T as the dz product's A operand: lane -> row c = 32 cb + (lane & 31), element j of k-step ks ->
  // o = 16 ks + 8 (lane >> 5) + j (o < 64: residual rows, else skip rows)
  for (int i = tid; i < 2 * C * C; i += 512) {
    const int o = i >> 6, c = i & 63;
    const float w = o < C ? a.wr[(size_t)o * C + c] : a.ws[(size_t)(o - C) * C + c];
    if constexpr (BF3) {  // [policy] three planes 1 KB apart
      unsigned short h, m, l;
      bf3_split1(w, h, m, l);
      const int at = ((((c >> 5) * 8 + (o >> 4)) * 3) * 64 + (c & 31) + 32 * ((o >> 3) & 1)) * 8 + (o & 7);
      wimg[at] = h;
      wimg[at + 512] = m;
      wimg[at + 1024] = l;
    } else {
      wimg[((((c >> 5) * 8 + (o >> 4)) * 64 + (c & 31) + 32 * ((o >> 3) & 1)) * 8) + (o & 7)] = b16_one(w);
    }
  }
  const unsigned wa0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned short *)wimg + 16u * lane;

  // ---- phase-2 roles (bwd_dx_wgfg64_kernel's): tap half, K half, channel block; B operand W_tap[o][32 wc + li]
  // for o = 64 kh + 16 j + 8 lh + e
  const int half = wave >> 2, kh = (wave >> 1) & 1, wc = wave & 1;
  u32x4 wp[4][BF3 ? 3 : 1];  // [policy] per k-step: the planes h, m, l, or the rounded values
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float wv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int o = 64 * kh + 16 * j + 8 * lh + e;
      const float *src = o < C ? a.wf : a.wg;
      wv[e] = src[((size_t)(o & (C - 1)) * C + 32 * wc + li) * 2 + (half ? 0 : 1)];
    }
    if constexpr (BF3)
      bf3_split8(wv, wp[j][0], wp[j][1], wp[j][2]);
    else
      wp[j][0] = b16_pack8(wv);
  }
  const int wm = wave >> 1, wn = wave & 1;  // filter / gate weight gradient: rows [32 wm, +32), columns [64 wn, +64)
  f32x16 accw[2], accr;                     // accr: residual / skip weight gradient, block (rows [32 wm, +32), channels [32 wn, +32))
#pragma unroll
  for (int r = 0; r < 16; ++r) accw[0][r] = accw[1][r] = accr[r] = 0.f;
  // phase-1 roles: dz block (channels [32 cb1, +32), steps [32 tq1, +32)) over the K half kh1 of the tile's 128 rows
  const int kh1 = wave >> 2, tq1 = (wave >> 1) & 1, cb1 = wave & 1;
  float *Zx = &O[C][0];  // the first K halves' partial dz (4 blocks x 16 x 64 floats) in the P0 staging rows, idle in phase 1

  // ---- staging: thread -> rows (tid >> 4) + 32 p, columns 4 (tid & 15) .. +3
  const int srow = tid >> 4, st = 4 * (tid & 15);
  f4 r_ga[2], r_gp[2], r_ds[2], r_th[2], r_sg[2], r_x[4];
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  // (GLOBAL only: row sums of df | dg, rows 32 p + srow; <false> never touches it and the compiler drops it)
  [[maybe_unused]] float gsum[GLOBAL ? 4 : 1] = {};
  bool z_ga = false, z_ds = false;  // the staged tile's dxo / dskip rows are absent (zeroed at the LDS store)
  const __amdgpu_buffer_rsrc_t gab = fb_rsrc(a.ga.p + (size_t)b * a.ga.sb);
  const __amdgpu_buffer_rsrc_t gpb = fb_rsrc(a.gp.p + (size_t)b * a.gp.sb);
  const __amdgpu_buffer_rsrc_t dskb = fb_rsrc(a.dskip.p + (size_t)b * a.dskip.sb);
  const __amdgpu_buffer_rsrc_t thb = fb_rsrc(a.th.p + (size_t)b * a.th.sb);
  const __amdgpu_buffer_rsrc_t sgb = fb_rsrc(a.sg.p + (size_t)b * a.sg.sb);
  const __amdgpu_buffer_rsrc_t xinb = fb_rsrc(a.xin.p + (size_t)b * a.xin.sb);
  const __amdgpu_buffer_rsrc_t oab = fb_rsrc(a.oa.p + (size_t)b * a.oa.sb);
  const __amdgpu_buffer_rsrc_t opb = fb_rsrc(a.op.p + (size_t)b * a.op.sb);
  [[maybe_unused]] __amdgpu_buffer_rsrc_t dfgb;  // WRITE_DFG: df | dg (B, 2C, Tp)
  if constexpr (WRITE_DFG) dfgb = fb_rsrc(a.dfg.p + (size_t)b * a.dfg.sb);
  // (every tensor but dskip is a (B, ch, Tp) view with the same row pitch -- checked by the launcher -- so one
  // per-lane offset and one scalar row pitch serve them all)
  const int vo_t = 4 * (srow * a.th.ld + st), vo_ds = 4 * (srow * a.dskip.ld + st);
  // a tile is INTERIOR when every operand row either covers it or misses it altogether (wave-uniform): raw
  // 16-byte buffer loads then; edge tiles take the masked form
  auto interior = [&](int t0) {
    const bool x_full = t0 >= a.t_lo && t0 + TT <= te;
    const bool ga_ok = !has_dxo || t0 >= a.up_lo || t0 + TT <= a.up_lo;
    const bool gp_ok = !has_dxo || t0 + TT + a.up_d <= a.t_end || t0 + a.up_d >= a.t_end;
    const bool s_ok = t0 >= skip_lo || t0 + TT <= skip_lo;
    return x_full && ga_ok && gp_ok && s_ok;
  };
  auto gload_r_part = [&](int t0, int part) {  // part 0..4: A', P0 (shifted), dskip, tanh, sigmoid of tile t0
    int ld_t = 4 * a.th.ld, ld_ds = 4 * a.dskip.ld;
    asm volatile("" : "+s"(ld_t), "+s"(ld_ds));  // (formed here, not hoisted)
    const int c4 = 4 * t0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (part == 0) {
        // (absent rows load a row that IS valid and are zeroed at the LDS store)
        r_ga[p] = (has_dxo && t0 >= a.up_lo) ? fb_load16(gab, vo_t, 32 * p * ld_t + c4) : fb_load16(thb, vo_t, c4);
      } else if (part == 1) {
        r_gp[p] = (has_dxo && t0 + a.up_d < a.t_end) ? fb_load16(gpb, vo_t, 32 * p * ld_t + c4 + 4 * a.up_d) : kZero4;
      } else if (part == 2) {
        r_ds[p] = t0 >= skip_lo ? fb_load16(dskb, vo_ds, 32 * p * ld_ds + c4 - 4 * a.t_base) : fb_load16(sgb, vo_t, c4);
      } else if (part == 3) {
        r_th[p] = fb_load16(thb, vo_t, 32 * p * ld_t + c4);
      } else {
        r_sg[p] = fb_load16(sgb, vo_t, 32 * p * ld_t + c4);
      }
    }
  };
  auto gload_r_edge = [&](int t0) {
    int srow_q = srow;
    asm volatile("" : "+v"(srow_q));
    const int t = t0 + st;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = 32 * p + srow_q;
      r_ga[p] = has_dxo ? ld4_edge(a.ga.at(b, row, 0), t, a.up_lo, te) : kZero4;
      r_gp[p] = has_dxo ? ld4_edge(a.gp.at(b, row, 0) + a.up_d, t, a.t_lo, min(a.t_end - a.up_d, te)) : kZero4;
    }
    if constexpr (BF3) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = 32 * p + srow_q;
      r_ds[p] = ld4_edge(a.dskip.at(b, row, 0) - a.t_base, t, skip_lo, te);
      r_th[p] = ld4_edge(a.th.at(b, row, 0), t, a.t_lo, te);
      r_sg[p] = ld4_edge(a.sg.at(b, row, 0), t, a.t_lo, te);
    }
  };
  auto set_zero_flags = [&](int t0, bool inter) {  // which row groups of tile t0 are absent (interior tiles only)
    z_ga = inter && (!has_dxo || t0 < a.up_lo);
    z_ds = inter && t0 < skip_lo;
  };
  auto gload_x = [&](int t0) {  // rows [0, 64): x(t - d); [64, 128): x(t)
    if (t0 >= a.t_lo && t0 + TT <= te) {
      int ld_x = 4 * a.th.ld;
      asm volatile("" : "+s"(ld_x));
#pragma unroll
      for (int p = 0; p < 4; ++p) r_x[p] = fb_load16(xinb, vo_t, 32 * (p & 1) * ld_x + 4 * t0 - (p < 2 ? 4 * a.d : 0));
    } else {
      int srow_q = srow;
      asm volatile("" : "+v"(srow_q));
      const int t = t0 + st;
#pragma unroll
      for (int p = 0; p < 4; ++p)
        r_x[p] = ld4_edge(a.xin.at(b, 32 * (p & 1) + srow_q, 0) - (p < 2 ? a.d : 0), t, a.t_lo, te);
    }
  };
  auto lstore_r = [&]() {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      // (absent A': P0 alone; P0 past the end of the sequence or no dxo at all: r_gp is zero)
      const f4 dxo = z_ga ? r_gp[p] : f4_add(r_ga[p], r_gp[p]);
      const f4 dsk = z_ds ? kZero4 : r_ds[p];
      *(f4 *)&U[32 * p + srow][st] = dxo;
      *(f4 *)&O[32 * p + srow][st] = dxo;
      *(f4 *)&U[C + 32 * p + srow][st] = dsk;
      bsum[p] += (dxo.x + dxo.y) + (dxo.z + dxo.w);  // bias gradients = row sums
      bsum[2 + p] += (dsk.x + dsk.y) + (dsk.z + dsk.w);
      *(f4 *)&Gt[32 * p + srow][st] = r_th[p];
      *(f4 *)&Gt[C + 32 * p + srow][st] = r_sg[p];
    }
  };
  auto row8 = [&](const float *row, float (&o)[8]) {  // 8 consecutive values of a row
    const f4 a0 = *(const f4 *)row, a1 = *(const f4 *)(row + 4);
    o[0] = a0.x; o[1] = a0.y; o[2] = a0.z; o[3] = a0.w; o[4] = a1.x; o[5] = a1.y; o[6] = a1.z; o[7] = a1.w;
  };
  typedef __attribute__((address_space(3))) u32x4 lds_u4;
#if MVN_EXP == 74  // (timing build: no MFMAs)
#define FBL_MF(acc_, a_, b_) acc_[0] += __uint_as_float(a_[0] ^ b_[0])
#else
#define FBL_MF(acc_, a_, b_) acc_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a_), __builtin_bit_cast(bf16x8, b_), acc_, 0, 0, 0)
#endif

  {
    const bool inter = interior(tb);
    if (inter) {
#pragma unroll
      for (int part = 0; part < 5; ++part) gload_r_part(tb, part);
    } else {
      gload_r_edge(tb);
    }
    set_zero_flags(tb, inter);
  }
  lstore_r();
  __syncthreads();  // (covers the weight image too)
#if MVN_EXP == 76  // (diagnostic build: cycles per section of a tile, summed over the workgroup's tiles, printed by two waves)
  unsigned tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = (unsigned)__builtin_readcyclecounter(), ntile = 0;
#define FBL_STAMP(i_) if constexpr (BF3) { const unsigned now_ = (unsigned)__builtin_readcyclecounter(); tsum[i_] += now_ - tlast; tlast = now_; }
#else
#define FBL_STAMP(i_)
#endif
  for (int t0 = tb; t0 < te; t0 += TT) {
    const bool more = t0 + TT < te;
    FBL_STAMP(7)
    if (ld_ok || t0 == tb) gload_x(t0);  // this tile's x rows fly under phase 1
    if constexpr (BF3) __builtin_amdgcn_sched_barrier(0);
    f32x16 accd;
#pragma unroll
    for (int r = 0; r < 16; ++r) accd[r] = 0.f;
    {
      // ---- phase 1: 12 slots
      //   slots 0-3:  dz (32 c x 32 t), this wave's K half = [Wr | Ws]^T (A: image in LDS) x [dxo; dskip] (B: read across
      //               the tile's rows), one k-step each;
      //   slots 4-11: residual / skip weight gradient, rows [32 wm, +32) of [dxo; dskip] x z^T (channels [32 wn, +32)),
      //               K = time: per 16 steps the row operand (even slot), then z = tanh x sigmoid (o x s) and the product
      if constexpr (BF3) {
        // [policy] software-pipelined like phase 2 (bf3_slot): slot s reads operand s + 1 (and the next k-step's weight
        // planes), then issues the MFMAs of operand s with its m and l planes and the h plane of operand s + 1 formed
        // behind them
        float ob[2][8], sgv[8];
        auto fetch1 = [&](int sI, float (&o)[8]) {
          if (sI < 4) {
            const int ks = 4 * kh1 + sI;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = U[16 * ks + 8 * lh + e][32 * tq1 + li];
          } else {
            const int G = (sI - 4) >> 1;
            if (((sI - 4) & 1) == 0) {
              const f4 a0 = *(const f4 *)&U[32 * wm + li][16 * G + 2 * h4], a1 = *(const f4 *)&U[32 * wm + li][16 * G + 2 * h4 + 4];
              o[0] = a0.x; o[1] = a0.y; o[2] = a0.z; o[3] = a0.w; o[4] = a1.x; o[5] = a1.y; o[6] = a1.z; o[7] = a1.w;
            } else {
              const f4 t0v = *(const f4 *)&Gt[32 * wn + li][16 * G + 2 * h4], t1v = *(const f4 *)&Gt[32 * wn + li][16 * G + 2 * h4 + 4];
              const f4 s0v = *(const f4 *)&Gt[C + 32 * wn + li][16 * G + 2 * h4], s1v = *(const f4 *)&Gt[C + 32 * wn + li][16 * G + 2 * h4 + 4];
              o[0] = t0v.x; o[1] = t0v.y; o[2] = t0v.z; o[3] = t0v.w; o[4] = t1v.x; o[5] = t1v.y; o[6] = t1v.z; o[7] = t1v.w;
              sgv[0] = s0v.x; sgv[1] = s0v.y; sgv[2] = s0v.z; sgv[3] = s0v.w; sgv[4] = s1v.x; sgv[5] = s1v.y; sgv[6] = s1v.z; sgv[7] = s1v.w;
            }
          }
        };
        u32x4 wA[2][3], hc, hn, mc, lc, ah, am, al;
        auto fetchA = [&](int sI, u32x4 (&w)[3]) {
          const unsigned wa = wa0 + 3072u * (unsigned)(cb1 * 8 + 4 * kh1 + sI);
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) w[pl] = *(const lds_u4 *)(uintptr_t)(wa + 1024u * pl);
        };
        fetch1(0, ob[0]);
        fetchA(0, wA[0]);
        bf3_peel(ob[0], hc);
        __builtin_amdgcn_sched_barrier(0);
#pragma clang loop unroll(full)
        for (int sI = 0; sI < 12; ++sI) {
          float (&xc)[8] = ob[sI & 1];
          float (&xn)[8] = ob[(sI + 1) & 1];
          if (sI + 1 < 12) fetch1(sI + 1, xn);
          if (sI + 1 < 4) fetchA(sI + 1, wA[(sI + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
          if (sI < 4) {
            const u32x4 &wh = wA[sI & 1][0], &wmid = wA[sI & 1][1], &wl = wA[sI & 1][2];
            bf3_slot(true, xc, xn, mc, lc, hn,
                     [&]() { FBL_MF(accd, wl, hc); }, [&]() { FBL_MF(accd, wmid, hc); }, [&]() { FBL_MF(accd, wh, hc); },
                     [&]() { FBL_MF(accd, wmid, mc); }, [&]() { FBL_MF(accd, wh, mc); }, [&]() { FBL_MF(accd, wh, lc); });
          } else if (((sI - 4) & 1) == 0) {
            // the row operand's planes; then z = tanh x sigmoid of the next slot and its h plane
            ah = hc;
            bf3_peel(xc, am);
            bf3_pack_l(xc, al);
#pragma unroll
            for (int e = 0; e < 8; ++e) xn[e] *= sgv[e];
            bf3_peel(xn, hn);
          } else {
            bf3_slot(sI + 1 < 12, xc, xn, mc, lc, hn,
                     [&]() { FBL_MF(accr, al, hc); }, [&]() { FBL_MF(accr, am, hc); }, [&]() { FBL_MF(accr, ah, hc); },
                     [&]() { FBL_MF(accr, am, mc); }, [&]() { FBL_MF(accr, ah, mc); }, [&]() { FBL_MF(accr, ah, lc); });
          }
          hc = hn;
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) Zx[(((2 * tq1 + cb1) * 2 + kh1) * 8 + r) * 64 + lane] = kh1 ? accd[r] : accd[8 + r];  // (hand-over, below)
      } else {
        // [policy] per slot: the LDS reads of the next operand, four conversions, ONE MFMA
        float ob[2][8], sgv[2][8];
        auto fetch1 = [&](int sI, float (&o)[8], float (&s)[8]) {
          if (sI < 4) {
            const int ks = 4 * kh1 + sI;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = U[16 * ks + 8 * lh + e][32 * tq1 + li];
          } else {
            const int G = (sI - 4) >> 1;
            if (((sI - 4) & 1) == 0) {
              row8(&U[32 * wm + li][16 * G + 2 * h4], o);
            } else {
              row8(&Gt[32 * wn + li][16 * G + 2 * h4], o);
              row8(&Gt[C + 32 * wn + li][16 * G + 2 * h4], s);
            }
          }
        };
        u32x4 wA[2], aq;
        auto fetchA = [&](int sI, u32x4 &w) { w = *(const lds_u4 *)(uintptr_t)(wa0 + 1024u * (unsigned)(cb1 * 8 + 4 * kh1 + sI)); };
        fetch1(0, ob[0], sgv[0]);
        fetchA(0, wA[0]);
#pragma clang loop unroll(full)
        for (int sI = 0; sI < 12; ++sI) {
          if (sI + 1 < 12) fetch1(sI + 1, ob[(sI + 1) & 1], sgv[(sI + 1) & 1]);
          if (sI + 1 < 4) fetchA(sI + 1, wA[(sI + 1) & 1]);
          float (&xc)[8] = ob[sI & 1];
          if (sI < 4) {
            B16_MFMA(accd, wA[sI & 1], b16_pack8(xc));
          } else if (((sI - 4) & 1) == 0) {
            aq = b16_pack8(xc);
          } else {
            float zv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) zv[e] = xc[e] * sgv[sI & 1][e];
            B16_MFMA(accr, aq, b16_pack8(zv));
          }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) Zx[(((2 * tq1 + cb1) * 2 + kh1) * 8 + r) * 64 + lane] = kh1 ? accd[r] : accd[8 + r];  // (hand-over, below)
      }
    }
    // (the hand-over that ends either policy's slots: the two K halves of a block meet through the P0 staging rows, each
    // wave handing over the HALF of its partial sums the other one finishes -- registers 8 (1 - kh1) .. +8 -- so that all
    // eight waves share the gate derivative.  It is written inside each policy's scope, twice: behind the scope, where the
    // slot loop's operand registers are already dead, the compiler packs the BF3 split differently and the fp32 kernels
    // no longer compile to what they compiled to.)
    if constexpr (BF3) __builtin_amdgcn_sched_barrier(0);
    FBL_STAMP(0)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the x rows (and the previous tile's stores)
    __syncthreads();  // B1: U and tanh | sigmoid have been read; the partial sums of dz are staged
    FBL_STAMP(1)
    {
      // ---- gate derivative in place: this lane holds dz of channels 32 cb1 + acc_row(r) at t = 32 tq1 + li, r in [8 kh1, +8)
      float tv[8], sv[8], dzv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int rr = 8 * kh1 + r, c = 32 * cb1 + (rr & 3) + 8 * (rr >> 2) + h4, tc = 32 * tq1 + li;
        tv[r] = Gt[c][tc];
        sv[r] = Gt[C + c][tc];
        dzv[r] = Zx[(((2 * tq1 + cb1) * 2 + (1 - kh1)) * 8 + r) * 64 + lane];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int rr = 8 * kh1 + r, c = 32 * cb1 + (rr & 3) + 8 * (rr >> 2) + h4, tc = 32 * tq1 + li;
        const float dz = dzv[r] + (kh1 ? accd[8 + r] : accd[r]);
        Gt[c][tc] = dz * sv[r] * (1.0f - tv[r] * tv[r]);
        Gt[C + c][tc] = dz * tv[r] * sv[r] * (1.0f - sv[r]);
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) *(f4 *)&U[32 * p + srow][st] = r_x[p];
    __syncthreads();  // B2: df | dg and the x rows are staged
    FBL_STAMP(2)
    if (WRITE_DFG && st_ok) {
      // the fp32, unrounded df | dg tile, columns [t_lo, te) only
      const int t = t0 + st;
      if (t >= a.t_lo && t + 3 < te) {
#pragma unroll
        for (int p = 0; p < 4; ++p) fb_store16(*(const f4 *)&Gt[32 * p + srow][st], dfgb, vo_t, 4 * (32 * p * a.th.ld + t0));
      } else {
        float *base = a.dfg.p + (size_t)b * a.dfg.sb + t;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (t + e >= a.t_lo && t + e < te) base[(size_t)(32 * p + srow) * a.dfg.ld + e] = Gt[32 * p + srow][st + e];
      }
    }
    if constexpr (GLOBAL) {
      // the label's term: this thread's share of the rows of df | dg (fp32, unrounded), columns [t_lo, te) only.  A
      // column outside is zero already -- its tanh, sigmoid, dxo and dskip were staged as zeros (ld4_edge), so
      // dz = 0 and df = dg = 0 x 0 -- but the mask costs an edge tile four compares and leaves nothing to a stale value.
      const int tg = t0 + st;
      const bool full = t0 >= a.t_lo && t0 + TT <= te;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f4 v = *(const f4 *)&Gt[32 * p + srow][st];
        if (!full) {
          v.x = (tg >= a.t_lo && tg < te) ? v.x : 0.f;
          v.y = (tg + 1 >= a.t_lo && tg + 1 < te) ? v.y : 0.f;
          v.z = (tg + 2 >= a.t_lo && tg + 2 < te) ? v.z : 0.f;
          v.w = (tg + 3 >= a.t_lo && tg + 3 < te) ? v.w : 0.f;
        }
        gsum[p] += (v.x + v.y) + (v.z + v.w);
      }
    }
    const bool spread = more && ld_ok && interior(t0 + TT);
    if (more && ld_ok && !spread) gload_r_edge(t0 + TT);
    if constexpr (BF3) __builtin_amdgcn_sched_barrier(0);
    // ---- phase 2: this wave's K half of its tap's product for both 32-step blocks, and its two blocks of the
    // filter / gate weight gradient; the next tile's loads in parts between the steps
    f32x16 accd2[2];
#pragma unroll
    for (int ub = 0; ub < 2; ++ub)
#pragma unroll
      for (int r = 0; r < 16; ++r) accd2[ub][r] = 0.f;
    {
      // 20 slots, five per 16 time steps: the weight gradient's row operand of dfg, its two x operands, then this wave's
      // k-step of the tap product for both 32-step blocks (operand read ACROSS the tile's rows)
      float xb[2][8];
      if constexpr (BF3) {
        // [policy] software-pipelined INSIDE the wave (r4c): slot s issues the LDS reads of operand s + 1, then the six MFMAs
        // of operand s with, behind them, the m and l planes of operand s and the h plane of operand s + 1 (bf3_slot): no
        // vector instruction stands in front of an MFMA it does not feed.
        auto fetch2 = [&](int sI, float (&o)[8]) {
          const int G = sI / 5, k = sI - 5 * G;
          if (k < 3) {
            const float *row = k == 0 ? &Gt[32 * wm + li][0] : &U[64 * wn + 32 * (k - 1) + li][0];
            const f4 a0 = *(const f4 *)(row + 16 * G + 2 * h4), a1 = *(const f4 *)(row + 16 * G + 2 * h4 + 4);
            o[0] = a0.x; o[1] = a0.y; o[2] = a0.z; o[3] = a0.w; o[4] = a1.x; o[5] = a1.y; o[6] = a1.z; o[7] = a1.w;
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = Gt[64 * kh + 16 * G + 8 * lh + e][32 * (k - 3) + li];
          }
        };
        u32x4 hc, hn, mc, lc, ah, am, al;
        fetch2(0, xb[0]);
        bf3_peel(xb[0], hc);
        __builtin_amdgcn_sched_barrier(0);
#pragma clang loop unroll(full)
        for (int sI = 0; sI < 20; ++sI) {
          const int G = sI / 5, k = sI - 5 * G;
          float (&xc)[8] = xb[sI & 1];
          if (sI + 1 < 20) fetch2(sI + 1, xb[(sI + 1) & 1]);
          if (spread && k == 0) {  // the next tile's loads in parts between the slots
            gload_r_part(t0 + TT, G);
            if (G == 3) gload_r_part(t0 + TT, 4);
          }
          __builtin_amdgcn_sched_barrier(0);  // (the reads stay in front; the planes formed from them wait where they are used)
          if (k == 0) {
            ah = hc;
            bf3_peel(xc, am);
            bf3_pack_l(xc, al);
            bf3_peel(xb[(sI + 1) & 1], hn);
          } else if (k < 3) {
            f32x16 &acc = accw[k - 1];
            bf3_slot(sI + 1 < 20, xc, xb[(sI + 1) & 1], mc, lc, hn,
                     [&]() { FBL_MF(acc, al, hc); }, [&]() { FBL_MF(acc, am, hc); }, [&]() { FBL_MF(acc, ah, hc); },
                     [&]() { FBL_MF(acc, am, mc); }, [&]() { FBL_MF(acc, ah, mc); }, [&]() { FBL_MF(acc, ah, lc); });
          } else {
            f32x16 &acc = accd2[k - 3];
            const u32x4 &wh = wp[G][0], &wmid = wp[G][1], &wl = wp[G][2];
            bf3_slot(sI + 1 < 20, xc, xb[(sI + 1) & 1], mc, lc, hn,
                     [&]() { FBL_MF(acc, hc, wl); }, [&]() { FBL_MF(acc, hc, wmid); }, [&]() { FBL_MF(acc, hc, wh); },
                     [&]() { FBL_MF(acc, mc, wmid); }, [&]() { FBL_MF(acc, mc, wh); }, [&]() { FBL_MF(acc, lc, wh); });
          }
          hc = hn;
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        // [policy]
        auto fetch2 = [&](int sI, float (&o)[8]) {
          const int G = sI / 5, k = sI - 5 * G;
          if (k < 3) {
            const float *row = k == 0 ? &Gt[32 * wm + li][0] : &U[64 * wn + 32 * (k - 1) + li][0];
            row8(row + 16 * G + 2 * h4, o);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = Gt[64 * kh + 16 * G + 8 * lh + e][32 * (k - 3) + li];
          }
        };
        u32x4 aq;
        fetch2(0, xb[0]);
#pragma clang loop unroll(full)
        for (int sI = 0; sI < 20; ++sI) {
          const int G = sI / 5, k = sI - 5 * G;
          if (sI + 1 < 20) fetch2(sI + 1, xb[(sI + 1) & 1]);
          if (spread && k == 0) {  // the next tile's loads in parts between the slots
            gload_r_part(t0 + TT, G);
            if (G == 3) gload_r_part(t0 + TT, 4);
          }
          const u32x4 xq = b16_pack8(xb[sI & 1]);
          if (k == 0) {
            aq = xq;
          } else if (k < 3) {
            B16_MFMA(accw[k - 1], aq, xq);
          } else {
            B16_MFMA(accd2[k - 3], xq, wp[G][0]);
          }
        }
      }
    }
    FBL_STAMP(3)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the next tile's loads, ahead of this tile's stores
    // ---- the K halves meet in O: rows [0, 64) hold dxo (tap 1: A' = dxo + W1^T dfg), rows [64, 128) take P0
    if (kh == 0) {
#pragma unroll
      for (int ub = 0; ub < 2; ++ub)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f4 *p4 = (f4 *)&O[64 * half + 32 * wc + li][32 * ub + 8 * q + h4];
          const f4 v = f4{accd2[ub][4 * q], accd2[ub][4 * q + 1], accd2[ub][4 * q + 2], accd2[ub][4 * q + 3]};
          *p4 = half ? v : f4_add(*p4, v);
        }
    }
    __syncthreads();  // B3: U and G have been read; the first K halves are in O
    FBL_STAMP(4)
    if (kh == 1) {
#pragma unroll
      for (int ub = 0; ub < 2; ++ub)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f4 *p4 = (f4 *)&O[64 * half + 32 * wc + li][32 * ub + 8 * q + h4];
          *p4 = f4_add(*p4, f4{accd2[ub][4 * q], accd2[ub][4 * q + 1], accd2[ub][4 * q + 2], accd2[ub][4 * q + 3]});
        }
    }
    __syncthreads();  // B4
    FBL_STAMP(5)
    if (st_ok) {
      // whole-row float4 stores: rows srow + 32 p (A' rows, then P0 rows), columns t0 + st .. +3 inside [t_lo, te)
      const int t = t0 + st;
      if (t >= a.t_lo && t + 3 < te) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          fb_store16(*(const f4 *)&O[32 * p + srow][st], oab, vo_t, 4 * (32 * p * a.th.ld + t0));
          fb_store16(*(const f4 *)&O[C + 32 * p + srow][st], opb, vo_t, 4 * (32 * p * a.th.ld + t0));
        }
      } else {
        float *ba = a.oa.p + (size_t)b * a.oa.sb + t, *bp = a.op.p + (size_t)b * a.op.sb + t;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (t + e >= a.t_lo && t + e < te) {
              ba[(size_t)(32 * p + srow) * a.oa.ld + e] = O[32 * p + srow][st + e];
              bp[(size_t)(32 * p + srow) * a.op.ld + e] = O[C + 32 * p + srow][st + e];
            }
      }
    }
    // (a thread's lstore_r() overwrites exactly the O elements the same thread has just read; U and G were
    // last read before B3)
    if (more) {
      set_zero_flags(t0 + TT, spread || !ld_ok);
      lstore_r();
    }
    __syncthreads();  // B5
    FBL_STAMP(6)
#if MVN_EXP == 76
    ++ntile;
#endif
  }
#undef FBL_MF
#undef FBL_STAMP
#if MVN_EXP == 76
  if (BF3 && blockIdx.x == 3 && (tid == 0 || tid == 320))
    printf("FBL wave %d tiles %u: phase1 %u | wait+B1 %u | gate+X %u | phase2 %u | wait+kh0+B3 %u | kh1+B4 %u | out+lstore+B5 %u | top %u\n",
           tid >> 6, ntile, tsum[0] / ntile, tsum[1] / ntile, tsum[2] / ntile, tsum[3] / ntile, tsum[4] / ntile, tsum[5] / ntile,
           tsum[6] / ntile, tsum[7] / ntile);
#endif
  // ---- this workgroup's slabs and bias partial sums (wgrad2_kernel's formats: 128 x 128, 128 x 64, 128)
  {
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int lane_e = tid_e & 63, wave_e = tid_e >> 6, wm_e = wave_e >> 1, wn_e = wave_e & 1;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = 32 * wm_e + acc_row(r, lane_e), n = 64 * wn_e + 32 * ni + (lane_e & 31);
        fg_part[((size_t)blockIdx.x * 128 + m) * 128 + n] = accw[ni][r];
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = 32 * wm_e + acc_row(r, lane_e), n = 32 * wn_e + (lane_e & 31);
      rs_part[((size_t)blockIdx.x * 128 + m) * 64 + n] = accr[r];
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float v = bsum[p];  // 16 lanes share a row
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    // bsum[p]: dxo rows 32 p + srow (p < 2), dskip rows 32 (p - 2) + srow
    if ((tid & 15) == 0) rs_bias_part[(size_t)blockIdx.x * 128 + (p < 2 ? 32 * p : C + 32 * (p - 2)) + srow] = v;
  }
  if constexpr (GLOBAL) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float v = gsum[p];  // 16 lanes share a row
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if ((tid & 15) == 0) g_part[(size_t)blockIdx.x * 128 + 32 * p + srow] = v;  // rows [0, 64): df, [64, 128): dg
    }
  }
}
