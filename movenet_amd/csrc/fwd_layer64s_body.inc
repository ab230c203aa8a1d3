// The body of every forward STRIP layer kernel (C = K = 64): the strip scaffold and, under `if constexpr`, the sections
// in which the kernels differ, each marked [policy].  Not a header of its own: it opens at the brace behind a kernel's
// parameter list (fused_bf16.h, in front of the LAYER_FORMS table, where every name below is in sight) and reads that
// kernel's names -- a, chunks_per_b, chunk_t and its template parameters -- under FS_FORM, the PRODUCT policy:
//   FS_FORM_F32    fused_layer64s_kernel<HAS_CTX>          fp32 MFMAs, weights staged from the parameter tensors
//   FS_FORM_BF3    fused_layer64s_bf3_kernel<GLOBAL>       bf16 x 3 (BF3_PRODUCT), three planes per weight
//   FS_FORM_BF16   fused_layer64s_bf16_kernel<GLOBAL, CTX> one bf16 plane (fb16_product)
//   FS_FORM_CTXW2  fused_layer64s_ctxw2_kernel             conditioned: x(t) and context on fp32 MFMAs, x(t - d) and
//                                                          the second product as planes
// The scaffold (described in fused_fwd.h): one WAVE owns a strip of 32 columns and runs the whole layer on it without
// a barrier; the strip's input goes from global memory into registers in ACCUMULATOR order and is the B operand; gate
// in registers; z in accumulator order is the second product's B operand.
{
  constexpr bool F32 = FS_FORM == FS_FORM_F32, BF3 = FS_FORM == FS_FORM_BF3, B16 = FS_FORM == FS_FORM_BF16,
                 CW2 = FS_FORM == FS_FORM_CTXW2;
#if FS_FORM == FS_FORM_F32
  constexpr bool GLOBAL = false, CTX = HAS_CTX;
#elif FS_FORM == FS_FORM_BF3
  constexpr bool CTX = false;
#elif FS_FORM == FS_FORM_CTXW2
  constexpr bool GLOBAL = false, CTX = true;
#endif
  static_assert(!(GLOBAL && CTX), "the label's bias form and the context form are separate kernels");
  // [policy] context operand.  fp32 MFMAs keep the context in the registers that otherwise fetch x(t) a strip ahead,
  // and load x(t) inside the strip; one plane has room for a third register block (xc) beside the prefetch
  constexpr bool CTX_IN_STRIP = CTX && !B16, CTX_BESIDE = CTX && B16;
  // pre-activation bias: bcf | bcg (CTX) or the label's vector (GLOBAL), added in front of tanh / sigmoid -- or, one
  // plane, the value the f | g accumulators start from: one LDS read per register and no add
  constexpr bool PRE_BIAS = (GLOBAL || CTX) && !B16, ACC_BIAS = (GLOBAL || CTX) && B16;
  // LDS: [x(t - d) planes (CW2)] | W1 | W2 | BI = br | bs | (bcf | bcg, or this sequence's gbias f | g rows); CW2 has
  // no room for BI and keeps the four vectors in registers
  constexpr int NK1 = CTX ? 24 : 16;  // F32: k-step groups of four per block of W1
  constexpr int XD_BYTES = CW2 ? FSC_XD_BYTES : 0;
  constexpr int W1_BYTES = F32 ? NK1 * 4096 : BF3 ? FS3_W1_BYTES : CW2 ? FSC_W1_BYTES : CTX ? FB16C_W1_BYTES : FB16_W1_BYTES;
  constexpr int W2_BYTES = F32 ? 32768 : B16 ? FB16_W2_BYTES : FS3_W2_BYTES;
  constexpr int IMG_BYTES = XD_BYTES + W1_BYTES + W2_BYTES + (CW2 ? 0 : CTX ? 256 * 4 : 128 * 4);
  extern __shared__ __attribute__((aligned(16))) unsigned char fs_lds[];
  float *BI = (float *)(fs_lds + W1_BYTES + W2_BYTES);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / chunks_per_b, ch = blockIdx.x - b * chunks_per_b;
  const int li = lane & 31, lh = lane >> 5;
  const int tb = (a.t_begin & ~TILE_ALIGN) + ch * chunk_t, te = min(a.t_end, tb + chunk_t);
  const int skip_lo = max(a.t_begin, a.t_skip0);

  // ---- [policy] weights into LDS: the image the form's pack kernel wrote once per forward call (a linear copy), or,
  // without one, converted here (bf16 x 3: 17 us per launch -- 48 dependent global load -> split -> three 2-byte LDS
  // stores per thread; the fp32 kernels' staging loops: ~8 us).  CW2 has the image only (plan_forward).
  if constexpr (F32) {
    // W1 [block][k-step / 4][lane][k-step % 4], k-steps x(t - d), x(t), context; W2 the same.  The loops run over the
    // SOURCE elements (coalesced reads of the (out, in, tap) / (out, in) tensors) and scatter into LDS.
    float *W1 = (float *)fs_lds, *W2 = (float *)(fs_lds + W1_BYTES);
    for (int sI = tid; sI < 2 * 8192; sI += 512) {
      const int g = sI >> 13, r = sI & 8191;        // g: 0 filter, 1 gate
      const int tap = r & 1, kc = (r >> 1) & 63, cm = r >> 7;
      const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3), kk = j + 32 * tap;
      const int blk = 2 * g + (cm >> 5), ln = (cm & 31) + 32 * lhs;
      W1[((blk * NK1 + (kk >> 2)) * 64 + ln) * 4 + (kk & 3)] = (g ? a.wg : a.wf)[r];
    }
    if (CTX) {
      for (int sI = tid; sI < 2 * 4096; sI += 512) {
        const int g = sI >> 12, r = sI & 4095;      // g: 0 filter, 1 gate context conv
        const int kc = r & 63, cm = r >> 6;
        const int lhs = (kc >> 2) & 1, kk = 64 + (kc & 3) + 4 * (kc >> 3);
        const int blk = 2 * g + (cm >> 5), ln = (cm & 31) + 32 * lhs;
        W1[((blk * NK1 + (kk >> 2)) * 64 + ln) * 4 + (kk & 3)] = (g ? a.wcg : a.wcf)[r];
      }
      if (tid < 128) BI[128 + tid] = tid < 64 ? a.bcf[tid] : a.bcg[tid - 64];
    }
    for (int sI = tid; sI < 2 * 4096; sI += 512) {
      const int g = sI >> 12, r = sI & 4095;        // g: 0 residual, 1 skip
      const int kc = r & 63, m2 = r >> 6;
      const int lhs = (kc >> 2) & 1, kk = (kc & 3) + 4 * (kc >> 3);
      const int blk = 2 * g + (m2 >> 5), ln = (m2 & 31) + 32 * lhs;
      W2[((blk * 8 + (kk >> 2)) * 64 + ln) * 4 + (kk & 3)] = (g ? a.ws : a.wr)[r];
    }
    if (tid < 128) BI[tid] = tid < 64 ? a.br[tid] : a.bs[tid - 64];
  } else if (CW2 || a.wpack) {
    LDS_IMAGE_COPY(fs_lds, a.wpack, IMG_BYTES);
  } else if constexpr (BF3) {
    fs3_stage_weights(fs_lds, a.wf, a.wg, a.wr, a.ws, a.br, a.bs, tid, 512);
  } else if constexpr (CTX) {
    fb16c_stage_weights(fs_lds, a.wf, a.wg, a.wr, a.ws, a.br, a.bs, a.wcf, a.wcg, a.bcf, a.bcg, tid, 512);
  } else {
    fb16_stage_weights(fs_lds, a.wf, a.wg, a.wr, a.ws, a.br, a.bs, tid, 512);
  }
  if constexpr (GLOBAL) {
    if (tid < 128) BI[128 + tid] = a.gbias[(size_t)b * 128 + tid];  // (f rows | g rows of this sequence)
  }
  __syncthreads();
  // this lane's 16 bytes of block 0, k-step 0 of each matrix
  const unsigned xda = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)fs_lds + 16u * lane;
  const unsigned w1a = xda + (unsigned)XD_BYTES;
  // (planes: two base registers per matrix, every plane is then within a ds_read's 16-bit offset of one of them)
  [[maybe_unused]] unsigned w1b = w1a + 2u * 8u * 3072u;
  // (F32: formed from the LDS address, not from w1a -- as w1a + 64 KB the constant is folded into the reads' offsets,
  // which it does not fit: an add per ds_read)
  unsigned w2a = F32 ? (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)(fs_lds + W1_BYTES) + 16u * lane
                     : w1a + (unsigned)W1_BYTES;
  [[maybe_unused]] unsigned w2b = w2a + 2u * 4u * 3072u;
  if constexpr (BF3) asm volatile("" : "+v"(w1b), "+v"(w2a), "+v"(w2b));
  if constexpr (CW2) asm volatile("" : "+v"(w2a), "+v"(w2b));
  // [policy] CW2: the bias vectors, one register each (lane i: element i), read with ds_bpermute
  [[maybe_unused]] int bv_r = 0, bv_s = 0, bv_cf = 0, bv_cg = 0;
  if constexpr (CW2) {
    bv_r = __float_as_int(a.br[lane]), bv_s = __float_as_int(a.bs[lane]);
    bv_cf = __float_as_int(a.bcf[lane]), bv_cg = __float_as_int(a.bcg[lane]);
  }
  // bias element c_ of vector i_ (0 br, 1 bs, 2 the f rows' pre-activation bias, 3 the g rows').  (A macro: as a
  // lambda it split a 16-byte LDS read of the one-plane GLOBAL / CTX forms in two and regrouped their gate arithmetic.)
#define FS_BIAS(i_, c_)                                                                                                       \
  (CW2 ? __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (c_), (i_) == 0 ? bv_r : (i_) == 1 ? bv_s : (i_) == 2 ? bv_cf : bv_cg)) \
       : BI[64 * (i_) + (c_)])
  typedef float fsv4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) fsv4 lds_v4;
  // channel of accumulator register r of block h in this lane: 32 h + (r & 3) + 8 (r >> 2) + 4 lh
  const int cbase = 4 * lh;

  // Every global access below is a raw BUFFER access: (a resource per tensor and sequence: four scalar registers) +
  // (row * ld: one scalar offset) + (one of five per-lane byte offsets).  Formed as 64-bit vector addresses the ~290
  // accesses of a strip spilled 443 registers; as scalar row pointers + vector offsets they still cost a 64-bit vector
  // add each and spilled the scalar file (130 v_writelane / v_readlane per strip).
  constexpr int RSRC = 0x00020000;  // raw buffer, 32-bit data format (gfx9)
  const __amdgpu_buffer_rsrc_t xb = __builtin_amdgcn_make_buffer_rsrc((void *)(a.xin.p + (size_t)b * a.xin.sb), 0, 0x7FFFFFFF, RSRC);
  const __amdgpu_buffer_rsrc_t thb = __builtin_amdgcn_make_buffer_rsrc((void *)(a.th.p + (size_t)b * a.th.sb), 0, 0x7FFFFFFF, RSRC);
  const __amdgpu_buffer_rsrc_t sgb = __builtin_amdgcn_make_buffer_rsrc((void *)(a.sg.p + (size_t)b * a.sg.sb), 0, 0x7FFFFFFF, RSRC);
  const __amdgpu_buffer_rsrc_t xob = __builtin_amdgcn_make_buffer_rsrc((void *)(a.xout.p + (size_t)b * a.xout.sb), 0, 0x7FFFFFFF, RSRC);
  const __amdgpu_buffer_rsrc_t skb = __builtin_amdgcn_make_buffer_rsrc((void *)(a.skip.p + (size_t)b * a.skip.sb - a.t_base), 0, 0x7FFFFFFF, RSRC);
  // CTX: the context (B, C, ctx_ld), column t = time t, read like the x(t) block (its own row pitch)
  // (formed here or behind the row pitches, as each form's own text had it: the other place moves scalar instructions)
  [[maybe_unused]] __amdgpu_buffer_rsrc_t cb;
  if constexpr (CTX_IN_STRIP) cb = __builtin_amdgcn_make_buffer_rsrc((void *)(a.ctx.p + (size_t)b * a.ctx.sb), 0, 0x7FFFFFFF, RSRC);
  const bool save = a.th.p != nullptr, has_out = a.xout.p != nullptr;
  // (row offsets = row * ld are re-formed where they are used, behind a fence on ld: hoisted out of the strip loop the
  // ~120 products filled the scalar file and were spilled to vector lanes)
  int xld4 = 4 * a.xin.ld, thld4 = 4 * a.th.ld, xold4 = 4 * a.xout.ld, skld4 = 4 * a.skip.ld;
  [[maybe_unused]] int cld4 = CTX_IN_STRIP ? 4 * a.ctx.ld : 0;
  if constexpr (CTX_BESIDE) {
    cb = __builtin_amdgcn_make_buffer_rsrc((void *)(a.ctx.p + (size_t)b * a.ctx.sb), 0, 0x7FFFFFFF, RSRC);
    cld4 = 4 * a.ctx.ld;
  }

  // x(t) of a strip (the tap-1 half of the input, 32 registers) is fetched one strip AHEAD, under the second product
  // of the strip before; the first product consumes it first, which gives the x(t - d) half, requested at the top of
  // the strip, the first half of the first product to arrive; the skip accumulator's old values arrive under the
  // second product in the x(t - d) registers.  (Without the prefetch the wave counters showed 51 % of the wave cycles
  // waiting for memory: a wave that issues MFMAs back to back starves the other wave of its SIMD, so the two fall into
  // step and wait together.)
  // (Tried, bf16 x 3: 8-byte stores -- a lane pair exchanges two registers by DPP so that one store instruction writes
  // 4 row segments of 128 bytes instead of 2, half the store instructions: 91.9 against 91.2 us, the stores cost their
  // bytes, not their count.  Tried: x(t - d) a strip ahead too and the old skip sums at the top of the strip, both as
  // initial values of the second product's accumulators: 17 us per layer SLOWER -- a wave has 64 vector-memory
  // instructions in flight at most (6-bit vmcnt), a strip issues 224, and 96 loads queued in front of the 64 stores of
  // the strip before stall the stores.)
  // (History: timing builds of the bf16 x 3 kernel, since removed, us per layer: all 92, no tanh / sigmoid stores 79,
  // no stores 65, no loads after a wave's first strip 78, neither 62, no MFMAs / splits 70.)
  auto column = [&](int t0_, bool &live_, int &tc_) {
    const int t_ = t0_ + li;
    live_ = t_ >= a.t_begin && t_ < te;
    tc_ = live_ ? t_ : a.t_begin;  // (clamped: dead lanes read a valid column, zeroed afterwards)
  };
  // the 32 rows of this lane's half of a block: register j <- channel (j & 3) + 8 (j >> 2) + 4 lh
#define FS_LOAD32(dst_, rsrc_, off_, ld4_)                                                                              \
  _Pragma("unroll") for (int j = 0; j < 32; ++j) dst_[j] =                                                              \
      __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc_, off_, ((j & 3) + 8 * (j >> 2)) * ld4_, 0))
#define FS_MASK32(dst_, live_) _Pragma("unroll") for (int j = 0; j < 32; ++j) dst_[j] = live_ ? dst_[j] : 0.f
  // (the same, each register masked as it is loaded)
#define FS_LOAD32_LIVE(dst_, rsrc_, off_, ld4_, live_)                                                                  \
  _Pragma("unroll") for (int j = 0; j < 32; ++j) {                                                                      \
    const float v_ = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc_, off_, ((j & 3) + 8 * (j >> 2)) * ld4_, 0)); \
    dst_[j] = live_ ? v_ : 0.f;                                                                                         \
  }
  float xb1[32];  // x(t) of the current strip: B operand of the first k-steps, residual input
  if constexpr (!CTX_IN_STRIP) {
    bool lv;
    int tcc;
    column(tb + 32 * wave, lv, tcc);
    const int o1 = 4 * (cbase * a.xin.ld + tcc);
    FS_FENCE(xld4);
    FS_LOAD32_LIVE(xb1, xb, o1, xld4, lv);
  }

  // Lanes that must not store (columns outside [t_begin, te), no output tensor) carry an offset beyond the buffer's
  // num_records: the hardware drops the access -- no exec-mask branch per store.
  // (Tried, fp32 MFMAs: holding a strip's x' and skip sums in registers until after the next strip's first product, so
  // that no wait on a prefetched load sits right behind 64 fresh stores -- on gfx9 loads and stores retire through one
  // in-order counter and the compiler's wait at the loop edge was vmcnt(0).  Measured 131.4 against 131.9 us per
  // layer: the second wave of the SIMD covers it.)
  constexpr int FS_OOB = (int)0x80000000;
  for (int t0 = tb + 32 * wave; t0 < te; t0 += 32 * 8) {
    const int t = t0 + li;
    bool live;
    int tc;
    column(t0, live, tc);
    const bool skip_live = t >= skip_lo && t < te;
    // per-lane byte offsets (channel part 4 lh of the row + the column)
    const int ox0 = 4 * (cbase * a.xin.ld + tc - a.d);
    const int oth = (save && live) ? 4 * (cbase * a.th.ld + tc) : FS_OOB, oxo = 4 * (cbase * a.xout.ld + tc);
    const int osk = 4 * (cbase * a.skip.ld + (skip_live ? t : skip_lo));
    float xn1[32];  // x(t) of the NEXT strip; CTX_IN_STRIP: ctx(t) of this one
    if constexpr (CTX_IN_STRIP) {  // [policy] x(t) and ctx(t) of this strip
      const int o1 = 4 * (cbase * a.xin.ld + tc), oc = 4 * (cbase * a.ctx.ld + tc);
      FS_FENCE(xld4);
      FS_FENCE(cld4);
      FS_LOAD32_LIVE(xb1, xb, o1, xld4, live);
      FS_LOAD32_LIVE(xn1, cb, oc, cld4, live);
    }
    // ---- x(t - d): B operand of the k-steps behind x(t)'s; later the skip accumulator's old values
    float xa0[32];
    FS_FENCE(xld4);
    FS_LOAD32(xa0, xb, ox0, xld4);
    // (interior strips -- wave-uniform test -- need no masking: 32 selects less per strip)
    if (!(t0 >= a.t_begin && t0 + 32 <= te)) FS_MASK32(xa0, live);
    // [policy] ctx(t) of this strip beside the prefetch (requested with x(t - d), consumed in a phase of its own behind
    // the audio product: the three operand blocks are never all live in bf16 form at once)
    [[maybe_unused]] float xc[CTX_BESIDE ? 32 : 1];
    if constexpr (CTX_BESIDE) {
      const int oc = 4 * (cbase * a.ctx.ld + tc);
      FS_FENCE(cld4);
      FS_LOAD32(xc, cb, oc, cld4);
      if (!(t0 >= a.t_begin && t0 + 32 <= te)) FS_MASK32(xc, live);
    }
    // ---- f | g: four 32 x 32 blocks (f c<32, f c>=32, g c<32, g c>=32), K = 128 (CTX: 192), the x(t) half first
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (ACC_BIAS)  // accumulator row = channel (r & 3) + 8 (r >> 2) + 4 lh of block i, the same in every lane
          acc[i][r] = BI[128 + 32 * i + (r & 3) + 8 * (r >> 2) + cbase];
        else
          acc[i][r] = 0.f;
      }
    // [policy] first product
    if constexpr (F32) {  // W1 [block][k-step / 4][lane][k-step % 4]: one ds_read_b128 feeds four MFMAs
#pragma unroll
      for (int kq = 0; kq < NK1; ++kq) {
        const int k4 = kq < 8 ? 8 + kq : kq < 16 ? kq - 8 : kq;  // x(t), x(t - d), context
        fsv4 aw[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) aw[blk] = *(const lds_v4 *)(uintptr_t)(w1a + 4u * (unsigned)((blk * NK1 + k4) * 256));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int blk = 0; blk < 4; ++blk)
            acc[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                aw[blk][e], k4 >= 16 ? xn1[4 * (k4 - 16) + e] : k4 >= 8 ? xb1[4 * (k4 - 8) + e] : xa0[4 * k4 + e], acc[blk], 0, 0, 0);
      }
    } else if constexpr (BF3) {
      BF3_PRODUCT(8, w1a, w1b, (ks_ < 4 ? xb1[8 * ks_ + e_] : xa0[8 * (ks_ - 4) + e_]));
    } else if constexpr (B16) {
      fb16_product<8, W1_BYTES / 4096>(acc, w1a, [&](int ks, int e) { return ks < 4 ? xb1[8 * ks + e] : xa0[8 * (ks - 4) + e]; });
      if constexpr (CTX) fb16_product<4, W1_BYTES / 4096, 8>(acc, w1a, [&](int ks, int e) { return xc[8 * ks + e]; });
    } else {  // CW2: x(t) (consumed first, fp32 MFMAs, groups 0..7 of 16), x(t - d) (planes at xda), context (groups 8..15)
#pragma unroll
      for (int kq = 0; kq < 16; ++kq) {
        if (kq == 8) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            u32x4 bh, bm, bl;
            bf3_split8(&xa0[8 * ks], bh, bm, bl);
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) bf3_mfma6(acc[blk], xda + 3072u * (unsigned)(blk * 4 + ks), bh, bm, bl);
          }
        }
        fsv4 aw[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) aw[blk] = *(const lds_v4 *)(uintptr_t)(w1a + 4u * (unsigned)((blk * 16 + kq) * 256));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int blk = 0; blk < 4; ++blk)
            acc[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[blk][e], kq >= 8 ? xn1[4 * (kq - 8) + e] : xb1[4 * kq + e], acc[blk], 0, 0,
                                                            0);
      }
    }
    // ---- gate in registers (fp32); tanh / sigmoid leave (written once, read by the backward pass much later: the
    // non-temporal hint); z in accumulator order = the next B operand
    float z[32];
    FS_FENCE(thld4);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c0 = 32 * h + (r & 3) + 8 * (r >> 2);
        // [policy] pre-activation bias.  (bf16 x 3 forms both sums ahead of tanh, the fp32-MFMA kernels each in front of
        // its function, as their own texts did: the other order moves the adds among the gate's instructions)
        float fv = acc[h][r], gv = acc[2 + h][r];
        if constexpr (PRE_BIAS && BF3) {
          fv += FS_BIAS(2, c0 + cbase);
          gv += FS_BIAS(3, c0 + cbase);
        }
        const float tv = tanh_fast(PRE_BIAS && !BF3 ? fv + FS_BIAS(2, c0 + cbase) : fv);
        const float sv = sigmoid_fast(PRE_BIAS && !BF3 ? gv + FS_BIAS(3, c0 + cbase) : gv);
        z[16 * h + r] = tv * sv;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(tv), thb, oth, c0 * thld4, FS_AUX_SAVE);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(sv), sgb, oth, c0 * thld4, FS_AUX_SAVE);
      }
    // the skip accumulator's old values, into the x(t - d) registers (dead now), and the NEXT strip's x(t), both under
    // the MFMAs below
    FS_FENCE(skld4);
    if (!a.first_layer) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          xa0[16 * h + r] = __uint_as_float(
              __builtin_amdgcn_raw_buffer_load_b32(skb, osk, (32 * h + (r & 3) + 8 * (r >> 2)) * skld4, 0));
    }
    if constexpr (!CTX_IN_STRIP) {
      if (t0 + 32 * 8 < te) {
        bool lv;
        int tcc;
        column(t0 + 32 * 8, lv, tcc);
        const int o1 = 4 * (cbase * a.xin.ld + tcc);
        FS_FENCE(xld4);
        FS_LOAD32(xn1, xb, o1, xld4);
        if (!(t0 + 32 * 8 >= a.t_begin && t0 + 32 * 8 + 32 <= te)) FS_MASK32(xn1, lv);
      } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) xn1[j] = 0.f;
      }
    }
    // ---- residual | skip: four blocks (res c<32, res c>=32, skip k<32, skip k>=32), K = 64
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    // [policy] second product
    if constexpr (F32) {
#pragma unroll
      for (int k4 = 0; k4 < 8; ++k4) {
        fsv4 aw[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) aw[blk] = *(const lds_v4 *)(uintptr_t)(w2a + 4u * (unsigned)((blk * 8 + k4) * 256));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int blk = 0; blk < 4; ++blk)
            acc[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[blk][e], z[4 * k4 + e], acc[blk], 0, 0, 0);
      }
    } else if constexpr (B16) {
      fb16_product<4>(acc, w2a, [&](int ks, int e) { return z[8 * ks + e]; });
    } else {
      BF3_PRODUCT(4, w2a, w2b, z[8 * ks_ + e_]);
    }
    // ---- x' = (y + br) + x(t): x(t) of this lane's channel is register 16 h + r of xb1;
    // skip (+)= y + bs, columns t - t_base, live from skip_lo
    FS_FENCE(xold4);
    FS_FENCE(skld4);
    {
      const int oxo_m = (has_out && live) ? oxo : FS_OOB, osk_m = skip_live ? osk : FS_OOB;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c0 = 32 * h + (r & 3) + 8 * (r >> 2);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((acc[h][r] + FS_BIAS(0, c0 + cbase)) + xb1[16 * h + r]), xob, oxo_m,
                                                c0 * xold4, 0);
        }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k0 = 32 * h + (r & 3) + 8 * (r >> 2);
          const float v = acc[2 + h][r] + FS_BIAS(1, k0 + cbase);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a.first_layer ? v : xa0[16 * h + r] + v), skb, osk_m, k0 * skld4, 0);
        }
    }
    if constexpr (!CTX_IN_STRIP) {
#pragma unroll
      for (int j = 0; j < 32; ++j) xb1[j] = xn1[j];
    }
  }
#undef FS_BIAS
#undef FS_LOAD32
#undef FS_MASK32
#undef FS_LOAD32_LIVE
}
