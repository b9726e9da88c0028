// resblock_body.h — the kernel text of resblock_bf16x3.hip's two kernels, included once per
// kernel (HFG_RB2 = 0: resblock_bf16x3, = 1: resblock2_bf16x3).  Not a header in its own
// right: it needs the declarations above its include site.
//
// Why an include and not a shared __device__ template: with the body behind a forceinline
// wrapper, 5 of the 12 persistent resblock_bf16x3 instances changed their register
// allocation (ResBlock2 section); included as text, the existing kernel is the
// function it was and compiles to the parent's figures.
//
// The body of both kernels.  RB2 = false: the reference's ResBlock (dilation pairs,
// resblock_bf16x3); RB2 = true: the public release's ResBlock2 (resblock2_bf16x3),
//   for m in dilations:  x = x + conv_m(lrelu(x))
// — the same window, operand planes, A stream (rb_pack, pack_layout.h, with n_dil convs) and
// epilogue; x stays in its registers across the convs and is the only tensor
// ever written as an operand, so a conv costs one operand rewrite instead of a pair's two.
#if HFG_RB2
template <int KT, int WAVES_M, int WAVES_N, int WM, int NP, int FMT>
__global__ void __launch_bounds__(64 * WAVES_M * WAVES_N, 2)  // 2 waves/SIMD: <= 256 VGPRs
resblock2_bf16x3(const RbParams p) {
  constexpr bool PERSIST = false;  // one window per block
  constexpr bool RB2 = true;
#else
template <int KT, int WAVES_M, int WAVES_N, int WM, int NP, int FMT, bool PERSIST>
__global__ void __launch_bounds__(64 * WAVES_M * WAVES_N, 2)  // 2 waves/SIMD: <= 256 VGPRs
resblock_bf16x3(const RbParams p) {
  constexpr bool RB2 = false;
#endif
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int NT = 64 * NW;
  static_assert(WM == 1 || WM == 2, "32 or 64 rows per wave");
  constexpr int C = 32 * WM * WAVES_M;
  constexpr int NG = C / 16;               // 16-channel groups
  constexpr int WN = 4 / WM;               // 32-column MFMA tiles per wave (WM row tiles)
  constexpr int NWIN = 32 * WN * WAVES_N;  // window columns
  constexpr int STEPS = NG * KT;           // MFMA k-steps per conv
  static_assert(STEPS % 2 == 0, "two-deep A register ring needs an even step count");
  // operand rows: the window plus MARG spare rows on each side, read by the taps of edge
  // columns: the first conv's operand fills its radius of them from x (write_margins), later
  // operands leave them stale (their contents only reach garbage columns)
  constexpr int MARG = rb_marg(C, NWIN);
  constexpr RbLds LY = rb_lds(C, NWIN);    // lds_layout.h
  constexpr int ROWS = LY.rows;
  constexpr int PS = LY.ps;                // bytes per plane: [row][8 bf16]
  constexpr int HPS = LY.hps;              // half-group (slots 0-7 | 8-15): hi, lo planes
  constexpr int GS = LY.gs;                // 16-channel group
  constexpr RbPack PK = rb_pack();         // the A strides (pack_layout.h), bytes
  constexpr int ASTEP = PK.step;           // bytes per k-step of one wave row-block (hi, lo)
  static_assert(LY.bias_off <= (int)kMaxLdsBytes, "operand planes");
  static_assert(C != 32 || (WM == 1 && 32 * LY.post_row * 4 <= LY.bias_off),
                "conv_post staging fits the operand planes");

  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* const bias_s = reinterpret_cast<float*>(lds + LY.bias_off);
  // f16x3: per-wave max |next operand| (NW floats after the biases)
  float* const amax_s = bias_s + p.n_conv * LY.bias_conv;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave % WAVES_M;
  const int wave_n = wave / WAVES_M;
  const int half = lane >> 5;
  const int col = lane & 31;
  // ---- windows: w = tile + n_tiles * item.  One window per block (grid n_tiles x B), or
  // with p.persist a grid of G blocks that walks the windows w, w + G, w + 2G, ... and issues
  // the next window's x and margin loads beside the current window's MRF read-modify-write
  // (one-block-per-CU instances: nothing else on the CU hides those round trips).  Windows past
  // an item's length are skipped (block-uniform). ----
  const int n_tiles = (p.L + p.W - 1) / p.W;
  const int n_win = n_tiles * p.batch;
  const int wstride = PERSIST ? (int)gridDim.x : n_win;
  auto item_of = [&](int wi) { return __builtin_amdgcn_readfirstlane(wi / n_tiles); };
  auto len_of = [&](int bi) { return p.len ? min(p.len[bi], p.L) : p.L; };
  auto valid = [&](int wi) {
    const int bi = item_of(wi);
    return (wi - bi * n_tiles) * p.W < len_of(bi);
  };
  int w = PERSIST ? (int)blockIdx.x : (int)(blockIdx.x + n_tiles * blockIdx.y);
  while (w < n_win && !valid(w)) {
    if (!PERSIST) return;  // whole block past this utterance's end (block-uniform)
    w += wstride;
  }
  if (w >= n_win) return;
  int b = item_of(w);
  int len_b = len_of(b);
  int t0 = (w - b * n_tiles) * p.W;
#if HFG_RB_TIMING
  const int ts_region = NWIN == 256 && C == 64 ? 18 + (p.conv0 > 0 ? 1 : 0)
                        : ((KT == 3 ? 0 : KT == 7 ? 1 : 2) * 3 + (C == 32 ? 0 : C == 64 ? 1 : 2)) * 2 +
                              (p.conv0 > 0 ? 1 : 0);
  const int ts_blk = blockIdx.y * gridDim.x + blockIdx.x;
  uint64_t* const ts = g_rb_ts + ((size_t)ts_region * kRbTs.blocks + (ts_blk < kRbTs.blocks ? ts_blk : 0)) * kRbTs.slots;
  // stamps kept in LDS (past the f16x3 maxima) and stored once at the end: a global (or
  // scratch) store mid-kernel would make every later vmcnt wait also wait for its write (one
  // in-order queue for vector loads and stores).  A persistent block keeps its last window's.
  uint64_t* const tsv = reinterpret_cast<uint64_t*>(amax_s + LY.amax_n);
  auto stamp = [&](int i) {
    const uint64_t t = __builtin_amdgcn_s_memtime();
    if (tid == 0) tsv[i] = t;
  };
  if (tid < kRbTs.slots) tsv[tid] = 0;
  __syncthreads();
  if (tid == 0) tsv[kRbTsStart] = __builtin_amdgcn_s_memrealtime();
  stamp(kRbTsSetup);
#else
  auto stamp = [](int) {};
#endif
  int ws = t0 - p.halo;
  const int cbase = wave_n * 32 * WN;      // first window column of this wave
  const int row0 = wave_m * 32 * WM;     // first row of this wave (WM row tiles of 32)
  const int n_conv = p.n_conv;
  // A stream: the whole ResBlock's convs (p.n_conv_stream per wave row-block); this launch
  // runs convs p.conv0 .. p.conv0 + n_conv - 1 of it (a ResBlock split into two launches)
  const int QT = p.n_conv_stream * STEPS;
  const int Q0 = p.conv0 * STEPS;
  const int dbg = p.dbg;
  auto rrow = [&](int r) { return acc_row(r, half); };

  for (int i = tid; i < n_conv * C; i += NT) bias_s[i] = p.bias[i];

  bool vk[WN];
  auto set_vk = [&]() {
#pragma unroll
    for (int k = 0; k < WN; ++k) vk[k] = (unsigned)(ws + cbase + 32 * k + col) < (unsigned)len_b;
  };
  set_vk();

  // ---- A stream (buffer loads: SGPR descriptor + scalar step offset, no address VALU) ----
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
  const int a_base = wave_m * WM * QT * ASTEP;  // row tile i: + i * QT * ASTEP
  const int a_lane = lane * PK.lane;
  bf16x8 ra_h[2][WM], ra_l[2][WM];
  auto load_a = [&](int slot, int q) {
    const int so = a_base + min(q, QT - 1) * ASTEP;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      ra_h[slot][i] = __builtin_bit_cast(
          bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, a_lane, so + i * QT * ASTEP, 0));
      ra_l[slot][i] = __builtin_bit_cast(
          bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, a_lane + PK.plane, so + i * QT * ASTEP, 0));
    }
  };
  load_a(0, Q0);
  load_a(1, Q0 + 1);
  stamp(kRbTsLoadsIssued);

  // ---- x and the MRF accumulator of utterance b through buffer descriptors ----
  // Element (row, column) sits at soffset = (row0 + row part of accumulator element r) * L * 4
  // (wave-uniform: SALU) + voffset = (4 * half * L + column) * 4 (one VGPR per column tile):
  // no per-element address VALU and no branches.  An item is fewer than 2^30 floats (the C
  // ABI's bound: a dword is dropped when voffset + soffset + 4 passes num_records, so a
  // 4-GiB item would lose its last float), so every offset and its dword end fit 32 bits;
  // the range is never relied on otherwise (masked lanes read offset 0).
  unsigned Lb = (unsigned)p.L * 4u;
  auto srow = [&](int i, int r) { return (unsigned)(row0 + 32 * i + acc_row(r)) * Lb; };
  const unsigned lrow = 4u * (unsigned)half * (unsigned)p.L;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.x + (int64_t)b * p.bs), 0, (int)0xFFFFFFFFu, 0x00020000);

  // ---- residual stream x: window -> registers (zero outside [0, len): masked after the wait) ----
  floatx16 xcur[WM][WN];
  auto issue_x = [&](floatx16 (&dst)[WM][WN], const __amdgpu_buffer_rsrc_t& rs, int wsx, int lenx) {
#pragma unroll
    for (int k = 0; k < WN; ++k) {
      const int gc = wsx + cbase + 32 * k + col;
      const unsigned vo = (unsigned)gc < (unsigned)lenx ? (lrow + (unsigned)gc) * 4u : 0u;
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          dst[i][k][r] = __builtin_bit_cast(
              float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, (int)srow(i, r), 0));
    }
  };
  auto mask_x = [&]() {
    // the ablation zeroes x after the loads (a select on a uniform flag inside the load
    // expression made the compiler branch per element)
    const bool xz = kAblate && (dbg & kAblRbZeroX);
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int k = 0; k < WN; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) xcur[i][k][r] = (vk[k] && !xz) ? xcur[i][k][r] : 0.f;
  };
  // ---- persistent grid: a window's x [C][ROWS] (columns ws - MARG ..) goes to the operand
  // planes' LDS by buffer-load-to-LDS (no VGPRs), issued beside the previous window's MRF
  // read-modify-write; the window then reads its x and margins from LDS.  The item's buffer
  // range (C * L floats) turns the columns outside it into zeros; columns outside [0, len)
  // are masked as in the register path. ----
  constexpr int XD_N = C * ROWS / 64;  // 64-dword pieces (ROWS % 4 == 0: C * ROWS % 64 == 0)
  static_assert(C * ROWS % 64 == 0 && C * ROWS * 4 == LY.bias_off, "x copy fills the operand planes");
  constexpr int XD_T = (XD_N + NW - 1) / NW;
  auto dma_x = [&](int wsx, int bi) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.x + (int64_t)bi * p.bs), 0, (int)(C * Lb), 0x00020000);
    int c = (wave * 64 + lane) / ROWS;
    int cl = wave * 64 + lane - c * ROWS;
#pragma unroll 4
    for (int q = 0; q < XD_T; ++q) {
      const int j = wave + NW * q;
      if (j < XD_N) {
        const unsigned vo = ((unsigned)c * (unsigned)p.L + (unsigned)(wsx - MARG + cl)) * 4u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t3)(lds + j * 256), 4, (int)vo, 0, 0,
                                                 0);
      }
      static_assert(64 * NW < 3 * ROWS, "two wraps at most");
      cl += 64 * NW;
      c += cl >= ROWS ? 1 : 0;
      cl -= cl >= ROWS ? ROWS : 0;
      c += cl >= ROWS ? 1 : 0;
      cl -= cl >= ROWS ? ROWS : 0;
    }
  };
  if constexpr (PERSIST) {
    dma_x(ws, b);
    wait_vm<0>();
    lds_barrier();
  } else {
    issue_x(xcur, xrs, ws, len_b);
  }
  // ---- the first conv's margins: operand columns [-R0, 0) and [NWIN, NWIN + R0) of the
  // window read from x (R0 = that conv's receptive-field radius <= MARG, host-checked), so the
  // first conv is exact on the whole window and the launch's halo leaves out its radius.  One
  // task = one column of one half-group: its 8 slot channels (write_operand's permutation) ----
  constexpr int MG_T = (4 * MARG * NG + NT - 1) / NT;  // margin tasks per thread
  const int R0 = (KT - 1) / 2 * p.dil[0];
  const int n_mg = 4 * R0 * NG;
  float mg[MG_T][8];
  auto mg_col = [&](int q, int wsx) {  // global column of margin task q (window origin wsx)
    const int t = tid + q * NT;
    const int m = (t >> 1) / NG;
    return wsx + (m < R0 ? m - R0 : NWIN + m - R0);
  };
  auto issue_mg = [&](float (&dst)[MG_T][8], const __amdgpu_buffer_rsrc_t& rs, int wsx, int lenx) {
#pragma unroll
    for (int q = 0; q < MG_T; ++q) {
      const int t = tid + q * NT;
      const int hh = t & 1, gq = (t >> 1) % NG;
      const int gc = mg_col(q, wsx);
      const bool ok = t < n_mg && (unsigned)gc < (unsigned)lenx;
      const unsigned vo = ok ? ((unsigned)(16 * gq + 4 * hh) * (unsigned)p.L + (unsigned)gc) * 4u : 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        dst[q][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                  rs, (int)vo, (int)(acc_row(e) * Lb), 0));
    }
  };
  auto mask_mg = [&]() {
#pragma unroll
    for (int q = 0; q < MG_T; ++q) {
      const int gc = mg_col(q, ws);
      const bool ok = tid + q * NT < n_mg && (unsigned)gc < (unsigned)len_b;
#pragma unroll
      for (int e = 0; e < 8; ++e) mg[q][e] = ok ? mg[q][e] : 0.f;
    }
  };
  if constexpr (!PERSIST) issue_mg(mg, xrs, ws, len_b);
  // persistent grid: x and the margins from the LDS copy
  auto read_x_lds = [&]() {
    const float* xl = reinterpret_cast<const float*>(lds);
    // the lane's base index, opaque per window: the loop-invariant addresses of the 16 x WM x WN
    // elements would otherwise be hoisted out of the window loop and held in VGPRs across it
    int xb = (row0 + 4 * half) * ROWS + MARG + cbase + col;
    asm volatile("" : "+v"(xb));
#pragma unroll
    for (int k = 0; k < WN; ++k)
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          xcur[i][k][r] = xl[xb + (32 * i + acc_row(r)) * ROWS + 32 * k];
#pragma unroll
    for (int q = 0; q < MG_T; ++q) {
      const int t = min(tid + q * NT, n_mg > 0 ? n_mg - 1 : 0);
      const int hh = t & 1, gq = (t >> 1) % NG, m = (t >> 1) / NG;
      const int cw = MARG + (m < R0 ? m - R0 : NWIN + m - R0);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        mg[q][e] = xl[(16 * gq + acc_row(e, hh)) * ROWS + cw];
    }
  };
  auto write_margins = [&](float sc) {
#pragma unroll
    for (int q = 0; q < MG_T; ++q) {
      const int t = tid + q * NT;
      if (t < n_mg) {
        const int hh = t & 1, gq = (t >> 1) % NG, m = (t >> 1) / NG;
        const int c = m < R0 ? m - R0 : NWIN + m - R0;  // window column
        const int off = gq * GS + hh * HPS + (c + MARG) * 16;
        bf16x8 h, l;
#pragma unroll
        for (int e = 0; e < 8; e += 2)
          split_into<FMT>(fmaxf(mg[q][e] * sc, mg[q][e] * (kLReluSlope * sc)),
                          fmaxf(mg[q][e + 1] * sc, mg[q][e + 1] * (kLReluSlope * sc)), h, l, e);
        *reinterpret_cast<bf16x8*>(lds + off) = h;
        *reinterpret_cast<bf16x8*>(lds + off + PS) = l;
      }
    }
  };

  // lane's byte address of window column (cbase + col) in its half-group's hi plane
  const int vb = half * HPS + (cbase + col + MARG) * 16;

  // leaky_relu and the zero padding as one max(v * f1, v * f2) per value: (1, 0.1) inside
  // [0, len) = bitwise max(v, 0.1 v), (0, 0) outside = 0 (3 VALU ops, no select; both
  // operands are products, so no canonicalising max of the raw value is needed)
  // (the factors are formed per write from vk: kept live across the kernel they cost the
  // C = 128 instance 16 VGPRs and spills)
  // B operand of the next conv: lrelu(v), zero outside [0, len), split hi/lo -> LDS.
  // The 8 accumulator rows a lane holds per 16-channel group are exactly the 8 slots
  // (one 16-B row of its half-group) it reads as a B fragment.
  // f16x3: the operand is scaled by sc = 2^e (block_exp) inside the same two factors
  // Two scalar v_mul_f32 per value, not one v_pk_mul_f32 per value pair (rounds 3-5): packed f32
  // VALU costs ~22 cycles more per instruction than its two scalar halves beside MFMAs
  // (MI355X_MICROARCH.md; same-box -0.9 % ResBlock time, profiles/r06/ab_rewrite.txt).
  auto write_operand = [&](const floatx16 (&v)[WM][WN], float sc) {
    if (kAblate && (dbg & kAblRbNoOperand)) return;
#pragma unroll
    for (int k = 0; k < WN; ++k) {
      const float f1 = vk[k] ? sc : 0.0f, f2 = vk[k] ? kLReluSlope * sc : 0.0f;
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int gg = 0; gg < 2; ++gg) {
          bf16x8 h, l;
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const float v0 = v[i][k][gg * 8 + e], v1 = v[i][k][gg * 8 + e + 1];
            split_into<FMT>(fmaxf(v0 * f1, v0 * f2), fmaxf(v1 * f1, v1 * f2), h, l, e);
          }
          char* dst = lds + (row0 / 16 + 2 * i + gg) * GS + vb + k * 512;
          *reinterpret_cast<bf16x8*>(dst) = h;
          *reinterpret_cast<bf16x8*>(dst + PS) = l;
        }
    }
  };
  // f16x3: the block's largest |value| over the window's exact columns sets the power-of-two
  // scale of each operand it writes (per block: the window of an item, and so the result, is
  // the same whatever else is in the batch).  Exact = inside [0, len) and at least `radius`
  // (the receptive-field radius of the convs run so far) from the window edges: the garbage
  // columns outside read the never-written margin rows (stale LDS), so counting them would
  // make the scale depend on earlier launches; garbage that overflows f16 stays in garbage
  // columns.  Each wave posts its max before the barrier that ends every read of the previous
  // operand, and all read the NW maxima after it.
  auto wave_amax = [&](const floatx16 (&v)[WM][WN], int radius, float m = 0.f) {
#pragma unroll
    for (int k = 0; k < WN; ++k) {
      const int c = cbase + 32 * k + col;
      float mk = 0.f;  // v_max3 over the column's 16 x WM rows, one select per column
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) mk = fmaxf(mk, fabsf(v[i][k][r]));
      m = (vk[k] && c >= radius && c < NWIN - radius) ? fmaxf(m, mk) : m;
    }
    m = wave_max(m);
    if (lane == 0) amax_s[wave] = m;
  };
  auto block_exp = [&]() {
    float m = amax_s[0];
#pragma unroll
    for (int w_ = 1; w_ < NW; ++w_) m = fmaxf(m, amax_s[w_]);
    return x3_exp(m);
  };

  // conv cv over the whole window: acc = bias + W_cv * operand (one LDS barrier at the
  // end: every wave has read the operand, which the caller then overwrites in place)
  floatx16 acc[WM][WN];
  auto run_conv = [&](int cv) {
    const int d = p.dil[cv];
    const int pad = (KT - 1) / 2 * d;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // f16x3: the bias joins after the unscale (finalize)
        const float bv = FMT == kFmtF16 ? 0.f : bias_s[cv * C + row0 + 32 * i + rrow(r)];
#pragma unroll
        for (int k = 0; k < WN; ++k) acc[i][k][r] = bv;
      }
    bf16x8 bh[2][WN], bl[2][WN];
    // step s = (group g, tap j): rows shifted by j*d - pad, one VALU add per step,
    // tiles / planes by immediate offsets
    auto load_b = [&](int buf, int s_) {
      const int g = s_ / KT, j = s_ - (s_ / KT) * KT;
      const char* src = lds + vb + (g * GS + (j * d - pad) * 16);
#pragma unroll
      for (int k = 0; k < WN; ++k) {
        bh[buf][k] = *reinterpret_cast<const bf16x8*>(src + k * 512);
        // ablation: no lo-plane reads (the hi fragment stands in; half the LDS reads)
        bl[buf][k] = (kAblate && (dbg & kAblRbNoLoB)) ? bh[buf][k]
                                               : *reinterpret_cast<const bf16x8*>(src + k * 512 + PS);
      }
    };
    const int qb = Q0 + cv * STEPS;
    prio_mfma();
    load_b(0, 0);
    // software pipeline: B fragments one step ahead (interleaved with this step's
    // MFMAs), A fragments two steps ahead
#pragma unroll
    for (int s_ = 0; s_ < STEPS; ++s_) {
      const int cur = s_ & 1;
      if (s_ + 1 < STEPS) load_b(cur ^ 1, s_ + 1);
#pragma unroll
      for (int k = 0; k < WN; ++k)
#pragma unroll
        for (int i = 0; i < WM; ++i)
          mma3<NP, FMT>(ra_h[cur][i], ra_l[cur][i], bh[cur][k], bl[cur][k], acc[i][k]);
      load_a(cur, qb + s_ + 2);
      if (s_ + 1 < STEPS) {
#pragma unroll
        for (int i = 0; i < 2 * WN; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
        }
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);    // 2 MFMA
      __builtin_amdgcn_sched_group_barrier(0x020, 2 * WM, 0);  // A loads
      __builtin_amdgcn_sched_group_barrier(0x008, NP * WM * WN, 0);  // rest of the MFMAs
      __builtin_amdgcn_sched_barrier(0);
    }
    prio_other();
  };
  // f16x3: acc = acc * 2^-(e_x + e_w) + bias (exact unscale, one rounding for the bias)
  int ex = 0;
  auto finalize = [&](int cv) {
    const float inv = exp2i(-(ex + p.ew[cv]));
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float bv = bias_s[cv * C + row0 + 32 * i + rrow(r)];
#pragma unroll
        for (int k = 0; k < WN; ++k) acc[i][k][r] = __builtin_fmaf(acc[i][k][r], inv, bv);
      }
  };

  const bool add = p.mrf_mode & 1;
  const bool div = p.mrf_mode & 2;
  // fused conv_post (C = 32, the network's last MRF write): the stage output is not stored;
  // it is computed on the centre plus the conv's radius 3 on either side and consumed from LDS
  const bool post = !RB2 && C == 32 && p.wav != nullptr;
  const int c_lo = post ? p.halo - 3 : p.halo, c_hi = post ? p.halo + p.W + 3 : p.halo + p.W;
  for (;;) {
    // persistent grid: the row offsets (16 x WM scalars) stay per-window values instead of
    // being hoisted out of the window loop and held (spilled) across it
    if constexpr (PERSIST) asm volatile("" : "+s"(Lb));
    // ---- this window's x (in flight, or in LDS) -> operand ----
    if constexpr (PERSIST) read_x_lds();
    mask_x();
    mask_mg();
    int radius = 0;  // f16x3: receptive-field radius of the convs run so far
    if constexpr (FMT == kFmtF16) {
#if HFG_RB_TIMING
      wait_vm<0>();
      stamp(kRbTsXLanded);
#endif
      float mm = 0.f;  // the margin columns are part of the first operand
#pragma unroll
      for (int q = 0; q < MG_T; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) mm = fmaxf(mm, fabsf(mg[q][e]));
      wave_amax(xcur, 0, mm);
      lds_barrier();
      ex = block_exp();
      stamp(kRbTsAmax);
    } else if (PERSIST) {
      lds_barrier();  // every wave has read x from LDS (the copy the operand overwrites)
    }
    write_operand(xcur, exp2i(ex));
    write_margins(exp2i(ex));
    lds_barrier();
    stamp(kRbTsPrologue);

    if constexpr (RB2) {
      // ResBlock2: x = x + (conv_m(lrelu(x)) + b_m); x is rewritten as the next conv's operand
      // (after the barrier that ends every wave's reads of the current one)
      for (int cv = 0; cv < n_conv; ++cv) {
        run_conv(cv);
        if constexpr (FMT == kFmtF16) {
          finalize(cv);
          if (cv > 0) radius += (KT - 1) / 2 * p.dil[cv];  // conv 0: exact (margins from x)
        }
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int k = 0; k < WN; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) xcur[i][k][r] = xcur[i][k][r] + acc[i][k][r];
        if (cv + 1 < n_conv) {
          if constexpr (FMT == kFmtF16) {
            wave_amax(xcur, radius);
            lds_barrier();
            ex = block_exp();
          } else {
            lds_barrier();
          }
          write_operand(xcur, exp2i(ex));
          lds_barrier();
        }
      }
    } else
    // dilation pairs: xt = lrelu(conv1(lrelu(x)) + b1); x = x + (conv2(xt) + b2)
    if constexpr (FMT == kFmtBf16) {
      for (int cv = 0; cv < n_conv; cv += 2) {
        run_conv(cv);
        lds_barrier();
        write_operand(acc, 1.0f);
        lds_barrier();
        run_conv(cv + 1);
        lds_barrier();
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int k = 0; k < WN; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) xcur[i][k][r] = xcur[i][k][r] + acc[i][k][r];
        if (cv + 2 < n_conv) {
          write_operand(xcur, 1.0f);
          lds_barrier();
        }
      }
    } else {
      for (int cv = 0; cv < n_conv; cv += 2) {
        run_conv(cv);
        stamp(kRbTsConv + 2 * cv);
        finalize(cv);
        if (cv > 0) radius += (KT - 1) / 2 * p.dil[cv];  // conv 0: exact (margins from x)
        wave_amax(acc, radius);
        lds_barrier();  // every wave is done reading the operand; the maxima are posted
        ex = block_exp();
        write_operand(acc, exp2i(ex));
        lds_barrier();
        stamp(kRbTsTrans + 2 * cv);
        run_conv(cv + 1);
        stamp(kRbTsConv + 2 * (cv + 1));
        finalize(cv + 1);
        radius += (KT - 1) / 2;  // conv2: dilation 1
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int k = 0; k < WN; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) xcur[i][k][r] = xcur[i][k][r] + acc[i][k][r];
        if (cv + 2 < n_conv) {
          wave_amax(xcur, radius);
          lds_barrier();
          ex = block_exp();
          write_operand(xcur, exp2i(ex));
          lds_barrier();
        }
        stamp(kRbTsTrans + 2 * (cv + 1));
      }
    }

    // ---- the next window of a persistent block (block-uniform) ----
    int wn = w + wstride;
    if constexpr (PERSIST)
      while (wn < n_win && !valid(wn)) wn += wstride;
    const bool more = PERSIST && wn < n_win;

    // ---- MRF: (mrf + x) [/ n_res] on the window centre ----
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.mrf + (int64_t)b * p.bs), 0, (int)0xFFFFFFFFu, 0x00020000);
    bool ok[WN];
    unsigned vo[WN];
#pragma unroll
    for (int k = 0; k < WN; ++k) {
      const int c = cbase + 32 * k + col;
      ok[k] = vk[k] && c >= c_lo && c < c_hi;
      vo[k] = ok[k] ? (lrow + (unsigned)(ws + c)) * 4u : 0u;
    }
    const bool skip_mrf = kAblate && (dbg & kAblRbNoMrf);  // ablation: no MRF epilogue
    // persistent grid: the next window's x copy is issued first, then the MRF loads, so the
    // two round trips overlap (one wait for both)
    int bn = b, len_n = len_b, wsn = ws;
    if (more) {
      bn = item_of(wn);
      len_n = len_of(bn);
      wsn = (wn - bn * n_tiles) * p.W - p.halo;
      lds_barrier();  // every wave is done reading the last conv's operand
      dma_x(wsn, bn);
    }
    // every MRF load is issued before any use (one wait for all 16 x WN), then the adds /
    // divisions for every tile; the empty asm keeps the compiler from sinking a tile's loads
    // into its store branch (which serialised one HBM round trip per element)
    // (the MRF values land in the accumulator registers, dead after the last conv: the
    // persistent variant has no VGPRs to spare for a separate set)
    floatx16 (&mv)[WM][WN] = acc;
    if (add && !skip_mrf) {
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int k = 0; k < WN; ++k)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            mv[i][k][r] = __builtin_bit_cast(
                float, __builtin_amdgcn_raw_buffer_load_b32(mrs, (int)vo[k], (int)srow(i, r), 0));
    }
    if (more) wait_vm<0>();  // the x copy (and the MRF values) have landed
    if (add && !skip_mrf) {
#if HFG_RB_TIMING
      wait_vm<0>();
      stamp(kRbTsMrfLanded);
#endif
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int k = 0; k < WN; ++k)
#pragma unroll
          for (int r = 0; r < 16; ++r) xcur[i][k][r] = mv[i][k][r] + xcur[i][k][r];
    }
    if (!skip_mrf) {
      if (div && p.mrf_rcp != 0.f) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int k = 0; k < WN; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) xcur[i][k][r] = div_fast(xcur[i][k][r], p.mrf_div, p.mrf_rcp);
      } else if (div) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int k = 0; k < WN; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) xcur[i][k][r] = xcur[i][k][r] / p.mrf_div;
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int k = 0; k < WN; ++k)
#pragma unroll
          for (int r = 0; r < 16; ++r) asm volatile("" ::"v"(xcur[i][k][r]));
      if constexpr (C == 32 && !RB2) {
        if (post) conv_post_tail<NT, NWIN, WN>(p, xcur, ok, lds, b, len_b, t0, tid, cbase, half, col);
      }
#pragma unroll
      for (int k = 0; k < WN; ++k) {
        if (ok[k] && !post) {
#pragma unroll
          for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              // through a scalar: __builtin_bit_cast of an ext_vector element lvalue compiled to
              // element 0 of the vector (every row stored the same value)
              const float v = xcur[i][k][r];
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), mrs, (int)vo[k], (int)srow(i, r), 0);
            }
        }
      }
      stamp(kRbTsConv + 2 * n_conv);
      if (p.amax_out) {  // f16x3 consumers of the stage output (block-uniform branch)
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < WN; ++k) {
          float mk = 0.f;
#pragma unroll
          for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) mk = fmaxf(mk, fabsf(xcur[i][k][r]));
          m = ok[k] ? fmaxf(m, mk) : m;
        }
        amax_commit(m, p.amax_out, b);
      }
    } else if (xcur[0][0][0] == 1.2345e-30f) {
      p.mrf[0] = xcur[WM - 1][WN - 1][15];
    }
    if (!more) break;
    // ---- advance: the next window's x becomes the residual stream ----
    w = wn;
    b = bn;
    len_b = len_n;
    ws = wsn;
    t0 = ws + p.halo;
    set_vk();
    load_a(0, Q0);
    load_a(1, Q0 + 1);
    lds_barrier();  // every wave's x pieces are in LDS (each waited for its own above)
  }
#if HFG_RB_TIMING
  if (tid == 0) {
    tsv[kRbTsTrans + 2 * n_conv] = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < kRbTs.slots; ++i) ts[i] = tsv[i];
  }
#endif
}

