// hifigan_capi.cpp — C ABI (include/hifigan_hip.h) and host orchestration of the
// MI355X HiFi-GAN Generator: parameter store keyed by the reference state_dict
// names, weight-norm folding, packing into the MFMA fragment order, workspace
// management and the 78-launch forward schedule of
// HiFiGANGenerator.forward (models/hifigan.py:224-261).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/hifigan_hip.h"
#include "../../include/hifigan_hip_inspect.h"
#include "kernels.h"

namespace hfg {
std::mutex& setup_mutex() {
  static std::mutex mu;
  return mu;
}
hipError_t ensure_max_lds(const void* fn) {
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(setup_mutex());
  if (done.count({fn, dev})) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e == hipSuccess) done.insert({fn, dev});
  return e;
}
}  // namespace hfg

using hfg::ConvParams;
using hfg::kTiles;
using hfg::TileCfg;
using hfg::TileId;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(HFG_EIO, "%s: %s", what, hipGetErrorString(e));
}

// Schedule overrides for A/B runs and the parity suites (hfg_debug_schedule_set): a
// process-wide table read when a handle is created.  The library reads no environment
// variable for its schedule, so a serving process runs the default schedule whatever it
// inherits.  Each knob: its valid range and what it selects.
struct SchedKnob {
  const char* name;
  int lo, hi;
};
constexpr SchedKnob kSchedKnobs[] = {
    {"FUSED_RB", 0, 1},     // whole-ResBlock kernels (0: layer by layer)
    {"FUSE_POST", 0, 1},    // conv_post + tanh inside the last C = 32 ResBlock launch
    {"RB_SPLIT", 0, 1},     // k = 11 whole-ResBlock launches split in two
    {"SMALL_TILE", -1, 1},  // small-grid tile: -1 auto, 0 never, 1 always
    {"RB_CONC", -1, 1},     // concurrent ResBlocks of small forwards: -1 auto, 0 off, 1 on
    {"UPS_FRAMES", 1, 2},   // output-frame upsampler: 1 when its grid fills the chip, 2 always
    {"SPLIT", 1, 2},        // batch halves on 2 HIP streams (1: one stream)
    {"RB_PERSIST", 0, 2},   // persistent C = 64 ResBlock grids: 0 off, 1 n_CU / 2, 2 n_CU
    {"DEBUG_FLAGS", 0, 1 << 30},  // kernel ablation bits (-DHFG_ABLATE=1 builds only)
    {"MEL_DFT", 0, 1},      // mel: the DFT-GEMM path instead of the FFT (mel_capi.cpp)
    {"AREG_TALL", 0, 1},    // 256-row layers on the 256x128 AREG tile (6) instead of tile 5
};
std::mutex g_sched_mu;
std::map<std::string, int> g_sched;

const SchedKnob* sched_knob(const char* name) {
  if (!name) return nullptr;
  for (const SchedKnob& k : kSchedKnobs)
    if (!strcmp(k.name, name)) return &k;
  return nullptr;
}

// the override of `knob` into *v if one is set (else *v is left alone)
void sched_apply(const char* knob, int* v) {
  std::lock_guard<std::mutex> lk(g_sched_mu);
  auto it = g_sched.find(knob);
  if (it != g_sched.end()) *v = it->second;
}
void sched_apply(const char* knob, bool* v) {
  int i = *v ? 1 : 0;
  sched_apply(knob, &i);
  *v = i != 0;
}

// models/hifigan.py:21-23
int get_padding(int k, int d) { return (int)((k * d - d) / 2); }

enum LayerKind { L_CONV, L_UPS, L_POST };

struct Layer {
  LayerKind kind;
  std::string mod;   // state_dict module prefix
  int C_in, C_out, k, dil, pad;
  int s, p;          // ConvTranspose1d stride / padding
  // GEMM view
  int M, KT, CK, tile, m_tiles, n_chunks;
  int prec;          // 0: fp32 MFMA kernel, 1: split-precision kernel (bf16x3 / f16x3)
  int ew = 0;        // f16x3: power-of-two exponent of this layer's weight packing
  size_t w_off, b_off;  // offsets (floats) into the packed device buffer
  size_t w_len, b_len;
  // bf16x3 layers: a second packing for the small-grid tile (kBf16x3SmallTile), -1: none
  int tile_s = -1, m_tiles_s = 0, n_chunks_s = 0;
  size_t ws_off = 0, bs_off = 0;
  // bf16x3 upsamplers with k = 2u: the output-frame kernel (ups_bf16x3.hip) on its own
  // packing, -1: none
  int ups_cfg = -1, m_tiles_f = 0;
  size_t wf_off = 0, bf_off = 0;
};

// f16x3, bf16x3 and bf16w run the split-operand MFMA kernels (f16x3 and bf16w in the f16
// format with power-of-two scales, bf16x3 in the bf16 format: bf16x3_common.h)
inline bool split_dtype(int dtype) {
  return dtype == HFG_DTYPE_F16X3 || dtype == HFG_DTYPE_BF16X3 || dtype == HFG_DTYPE_BF16W;
}
// (the exact-fp32 mode has no split format: -1, no scale slots)
inline int split_fmt(int dtype) {
  return dtype == HFG_DTYPE_BF16X3 ? hfg::kFmtBf16 : split_dtype(dtype) ? hfg::kFmtF16 : -1;
}

struct Param {
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool set = false;
};

struct ProfRec {
  const char* label;
  double flop, bytes;
  hipEvent_t e0, e1;
  int fwd, part, seq;  // forward call, batch half (0/1), launch index inside that half
};

// One ResBlock run by resblock_bf16x3 (whole block per launch): its packed A stream
// [wave_m][conv][group][tap][plane][lane][8] and biases [conv][C] in the packed buffer.
struct RbFused {
  std::vector<int> convs;     // layer indices in execution order conv1_0, conv2_0, conv1_1, ...
  bool fused = false;         // this ResBlock runs as one resblock_bf16x3 launch
  int kt = 0, halo = 0, W = 0, nwin = 0, wm = 1;  // window columns, row tiles per wave
  // split into two launches (convs [0, split) then [split, n)): each part's window pays
  // only its own receptive-field halo; the first writes x to scratch (0: one launch)
  int split = 0;
  int halo_p[2] = {0, 0}, W_p[2] = {0, 0};
  size_t w_off = 0, w_len = 0, b_off = 0, b_len = 0;  // in floats
};

struct Stage {
  int C = 0;                  // channels of this stage's MRF
  int conv_ups = -1;          // index of the ups layer (-1 in an MRF-only handle)
  std::vector<int> conv1;     // [j*n_dil + m]
  std::vector<int> conv2;
  std::vector<RbFused> rbs;   // per ResBlock: whole-block launch or layer by layer
  // thin stage (C <= 16): the whole MRF in one mrf_thin launch (packed-fp32 VALU)
  bool thin = false;
  std::vector<int> thin_convs;   // layer indices: conv1_0, conv2_0, conv1_1, ... per ResBlock
  std::vector<int> thin_conv0;   // ResBlock j runs thin_convs[thin_conv0[j] .. thin_conv0[j+1])
  std::vector<int> thin_halo;    // per ResBlock receptive-field radius
  std::vector<size_t> thin_w_off;  // per conv, floats into the packed buffer ([tap][ci][co])
  size_t thin_b_off = 0;           // [conv][C]
  // bf16x3: the MFMA kernel's A stream [conv][step][plane][lane][8] (mrf_thin_mfma.hip)
  bool thin_mfma = false;
  size_t thin_m_off = 0;           // floats into the packed buffer
  size_t thin_m_bytes = 0;
  std::vector<int> thin_m_conv;    // byte offset of each conv inside the stream
};

}  // namespace

struct hfg_handle {
  hfg_config cfg;
  int device;  // -1: host-only handle (validation / packing inspection)
  // MRF-only handle (hfg_mrf_create): one stage of ResBlocks keyed "resblocks.{j}.*"
  // (the MRF module's own state_dict), no conv_pre / ups / conv_post
  bool mrf_only = false;
  // one forward at a time per handle: the split stream, its fork/join events and the
  // profiling records are shared state (ctypes releases the GIL around the call)
  std::recursive_mutex mu;
  std::vector<Layer> layers;
  int conv_pre = -1, conv_post = -1;
  std::vector<Stage> stages;
  std::map<std::string, Param> params;       // "<mod>.weight" / "<mod>.bias"
  std::map<std::string, Param> wn_parts;     // "<mod>.weight_g" / "<mod>.weight_v"
  std::vector<std::string> param_order;
  bool dirty = true;
  std::vector<float> packed_host;
  float* packed_dev = nullptr;
  size_t packed_dev_len = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  bool profiling = false;
  bool use_fused_rb = true;  // whole-ResBlock kernel for C in {32, 64, 128} (HFG_FUSED_RB=0:
                             // layer by layer; the parity suites compare both schedules)
  bool rb_split = true;      // whole-ResBlock split in two launches where it cuts >= 10 % of the
                             // halo recompute (k = 11 in V1; HFG_RB_SPLIT=0: one launch)
  bool fuse_post = true;     // conv_post + tanh inside the last C = 32 ResBlock launch
                             // (HFG_FUSE_POST=0: its own kernel; bitwise the same wav)
  int ups_frames = 1;        // k = 2u upsamplers on the output-frame kernel: 1 when its grid
                             // fills the chip, 2 always (HFG_UPS_FRAMES; the polyphase
                             // conv1d_bf16x3 path gives the bitwise same result)
  int fmt = 0;               // split format of the split kernels (bf16x3_common.h)
  int np = 3;                // MFMA products per multiply-add: 3, or 2 (bf16w: lo(w) = 0)
  int small_tile = -1;       // small-grid tile: -1 auto (grid < kSmallGridBlocks), 0 never,
                             // 1 always (HFG_SMALL_TILE; bitwise invisible)
  int dbg_flags = 0;  // HFG_DEBUG_FLAGS (kernel ablations, -DHFG_ABLATE=1 builds only)
  // HFG_RB_PERSIST (default 2): persistent grids for the one-block-per-CU ResBlock launches
  int rb_persist = 2;
  // AREG_TALL: layers whose rows are a multiple of 256 on the 256x128 AREG tile (6): each input
  // window staged once per 128 output columns instead of once per m-tile (bitwise tile 5)
  int areg_tall = 1;
  int n_cu = 256;      // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  int halves = 1;      // batch halves of the running forward (2: two streams share the CUs)
  // batch split over two HIP streams (HFG_SPLIT=1 disables): the two halves' launches
  // overlap, so one half's ramp-down / epilogue tail runs beside the other's main loops
  int split = 2;
  static constexpr int64_t kSplitMinFrames = 4096;  // batch frames from which a forward runs as
                                                    // two halves on two streams
  hipStream_t aux = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  // concurrent ResBlocks of small forwards (HFG_RB_CONC: -1 auto, 0 off, 1 whenever the
  // workspace allows): per batch part, aux streams for ResBlocks 1.. and their events
  int rb_conc = -1;
  hipStream_t rb_aux[2][HFG_MAX_RES] = {};
  hipEvent_t rb_fork[2] = {};
  hipEvent_t rb_join[2][HFG_MAX_RES] = {};
  int fwd_count = 0;
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> event_pool;
};

namespace {

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

int validate_config(const hfg_config* c) {
  if (!c) return fail(HFG_EINVAL, "config is NULL");
  if (c->n_mels <= 0) return fail(HFG_EINVAL, "n_mels must be > 0");
  if (c->n_up <= 0 || c->n_up > HFG_MAX_STAGES) return fail(HFG_EINVAL, "n_up out of range");
  if (c->n_res <= 0 || c->n_res > HFG_MAX_RES) return fail(HFG_EINVAL, "n_res out of range");
  if (c->dtype != HFG_DTYPE_FP32 && !split_dtype(c->dtype))
    return fail(HFG_EINVAL, "dtype must be HFG_DTYPE_FP32 (0), HFG_DTYPE_BF16X3 (1), "
                "HFG_DTYPE_BF16W (2) or HFG_DTYPE_F16X3 (3)");
  if (c->c0 <= 0) return fail(HFG_EINVAL, "upsample_initial_channel must be > 0");
  if (c->resblock_type != 0 && c->resblock_type != 1)
    return fail(HFG_EINVAL, "resblock_type must be 0 (the reference's ResBlock) or 1 (ResBlock2), "
                "got %d", c->resblock_type);
  // the kernels' leaky_relu is max(v, s v): s < 1
  if (!std::isfinite(c->post_slope) || c->post_slope < 0.f || c->post_slope >= 1.f)
    return fail(HFG_EINVAL, "post_slope must be finite and in [0, 1) (0 = the reference's 0.1), "
                "got %g", (double)c->post_slope);
  for (int i = 0; i < c->n_up; ++i) {
    if (c->up_rates[i] <= 0 || c->up_kernels[i] <= 0)
      return fail(HFG_EINVAL, "upsample rate/kernel %d must be > 0", i);
    if ((c->c0 >> (i + 1)) <= 0) return fail(HFG_EINVAL, "channels vanish at stage %d", i);
  }
  for (int i = 0; i < c->n_up; ++i)
    if (c->up_kernels[i] < c->up_rates[i])
      // ConvTranspose1d(padding=(k-u)//2 < 0): torch raises "negative padding is not supported"
      return fail(HFG_EINVAL, "ups.%d: kernel %d < stride %d gives negative padding (k-u)//2; "
                  "negative padding is not supported", i, c->up_kernels[i], c->up_rates[i]);
  for (int j = 0; j < c->n_res; ++j) {
    if (c->res_kernels[j] <= 0) return fail(HFG_EINVAL, "resblock kernel %d must be > 0", j);
    if (c->res_kernels[j] % 2 == 0)
      // convs2 (dilation 1, padding get_padding(k, 1) = (k-1)//2) shortens the sequence by
      // one, so the reference's residual add x + xt (models/hifigan.py:85) fails
      return fail(HFG_EINVAL, "resblock %d: even kernel size %d is not length-preserving "
                  "(the reference's residual add x + xt fails on the size mismatch)", j,
                  c->res_kernels[j]);
    if (c->n_dil[j] <= 0 || c->n_dil[j] > HFG_MAX_DIL)
      return fail(HFG_EINVAL, "resblock %d dilation count out of range", j);
    for (int m = 0; m < c->n_dil[j]; ++m)
      if (c->dil[j][m] <= 0) return fail(HFG_EINVAL, "dilation must be > 0");
  }
  return HFG_OK;
}

void add_param(hfg_handle* h, const std::string& key, std::vector<int64_t> shape) {
  Param p;
  p.shape = std::move(shape);
  h->params[key] = std::move(p);
  h->param_order.push_back(key);
}

int add_conv(hfg_handle* h, LayerKind kind, const std::string& mod, int cin, int cout, int k,
             int dil, int pad) {
  Layer L{};
  L.kind = kind;
  L.mod = mod;
  L.C_in = cin;
  L.C_out = cout;
  L.k = k;
  L.dil = dil;
  L.pad = pad;
  L.M = cout;
  L.KT = k;
  h->layers.push_back(L);
  add_param(h, mod + ".weight", {cout, cin, k});
  add_param(h, mod + ".bias", {cout});
  return (int)h->layers.size() - 1;
}

// The ResBlock convs of one MRF (models/hifigan.py:96-114 / ResBlock.__init__ :34-70),
// state_dict keys "<pre>resblocks.{j}.convs{1,2}.{m}".
Stage build_stage(hfg_handle* h, int ch, const std::string& pre) {
  const hfg_config& c = h->cfg;
  Stage st;
  st.C = ch;
  for (int j = 0; j < c.n_res; ++j) {
    const int kr = c.res_kernels[j];
    const std::string rb = pre + "resblocks." + std::to_string(j);
    if (c.resblock_type == 1) {
      // ResBlock2: one conv per dilation, "<pre>resblocks.{j}.convs.{m}" (kept in conv1)
      for (int m = 0; m < c.n_dil[j]; ++m)
        st.conv1.push_back(add_conv(h, L_CONV, rb + ".convs." + std::to_string(m), ch, ch, kr,
                                    c.dil[j][m], get_padding(kr, c.dil[j][m])));
      continue;
    }
    for (int m = 0; m < c.n_dil[j]; ++m)
      st.conv1.push_back(add_conv(h, L_CONV, rb + ".convs1." + std::to_string(m), ch, ch, kr,
                                  c.dil[j][m], get_padding(kr, c.dil[j][m])));
    for (int m = 0; m < c.n_dil[j]; ++m)
      st.conv2.push_back(add_conv(h, L_CONV, rb + ".convs2." + std::to_string(m), ch, ch, kr, 1,
                                  get_padding(kr, 1)));
  }
  return st;
}

// Build the layer list in the order of HiFiGANGenerator.__init__ (models/hifigan.py:177-222)
// (an MRF-only handle: the one MRF).  Returns HFG_EINVAL when a layer's taps x dilation is
// beyond every kernel's staging limits.
int build_layers(hfg_handle* h) {
  const hfg_config& c = h->cfg;
  if (h->mrf_only) {
    h->stages.push_back(build_stage(h, c.c0 >> 1, ""));
  } else {
    h->conv_pre = add_conv(h, L_CONV, "conv_pre", c.n_mels, c.c0, 7, 1, 3);
    std::vector<int> ups_idx;
    for (int i = 0; i < c.n_up; ++i) {
      const int cin = c.c0 >> i, cout = c.c0 >> (i + 1);
      const int u = c.up_rates[i], k = c.up_kernels[i];
      Layer L{};
      L.kind = L_UPS;
      L.mod = "ups." + std::to_string(i);
      L.C_in = cin;
      L.C_out = cout;
      L.k = k;
      L.dil = 1;
      L.s = u;
      L.p = (k - u) / 2;  // models/hifigan.py:201 — Python floor division
      if (k - u < 0 && (k - u) % 2 != 0) L.p -= 1;
      L.M = cout * u;
      L.KT = (k + u - 1) / u;  // taps per output phase
      h->layers.push_back(L);
      ups_idx.push_back((int)h->layers.size() - 1);
      add_param(h, L.mod + ".weight", {cin, cout, k});
      add_param(h, L.mod + ".bias", {cout});
    }
    for (int i = 0; i < c.n_up; ++i) {
      Stage st = build_stage(h, c.c0 >> (i + 1), "mrfs." + std::to_string(i) + ".");
      st.conv_ups = ups_idx[i];
      h->stages.push_back(std::move(st));
    }
    h->conv_post = add_conv(h, L_POST, "conv_post", c.c0 >> c.n_up, 1, 7, 1, 3);
  }

  // GEMM tiling and packed-buffer offsets
  size_t off = 0;
  for (auto& L : h->layers) {
    if (L.kind == L_POST) {
      L.w_off = off;
      L.w_len = (size_t)L.C_in * 7;
      off += (L.w_len + 63) & ~(size_t)63;
      L.b_off = off;
      L.b_len = 1;
      off += 64;
      continue;
    }
    if (split_dtype(h->cfg.dtype) && (L.kind == L_CONV || L.kind == L_UPS) &&
        hfg::bf16x3_tile_for_rows(L.M) >= 0 && hfg::bf16x3_supported(L.KT, L.dil)) {
      // split-precision path: chunk = 16 channels x TPC taps
      L.tile = hfg::bf16x3_tile_for_rows(L.M);
      // tile 3 with the A fragments in registers (same packing): layer convs whose tap
      // count has a compile-time instance, whole 16-channel groups
      if (L.tile == 3 && L.kind == L_CONV && L.C_in % 16 == 0 &&
          (L.KT == 3 || L.KT == 5 || L.KT == 7 || L.KT == 11))
        L.tile = h->areg_tall && L.M % hfg::kBf16x3Tiles[hfg::kAregTallTile].MT() == 0
                     ? hfg::kAregTallTile
                     : hfg::kAregTile;
      const hfg::Bf16x3Cfg& t3 = hfg::kBf16x3Tiles[L.tile];
      L.prec = 1;
      L.CK = hfg::kBf16x3Ck;
      L.m_tiles = (L.M + t3.MT() - 1) / t3.MT();
      L.n_chunks = ((L.C_in + L.CK - 1) / L.CK) * ((L.KT + t3.TPC - 1) / t3.TPC);
      const size_t slab_bf16 = (size_t)t3.TPC * 2 * t3.MT() * 16;
      L.w_off = off;
      L.w_len = (size_t)L.m_tiles * L.n_chunks * slab_bf16 / 2;  // in floats
      off += (L.w_len + 63) & ~(size_t)63;
      L.b_off = off;
      L.b_len = (size_t)L.m_tiles * t3.MT();
      off += (L.b_len + 63) & ~(size_t)63;
      if (L.tile != hfg::kBf16x3SmallTile && L.M >= 64) {
        const hfg::Bf16x3Cfg& ts = hfg::kBf16x3Tiles[hfg::kBf16x3SmallTile];
        L.tile_s = hfg::kBf16x3SmallTile;
        L.m_tiles_s = (L.M + ts.MT() - 1) / ts.MT();
        L.n_chunks_s = ((L.C_in + L.CK - 1) / L.CK) * ((L.KT + ts.TPC - 1) / ts.TPC);
        L.ws_off = off;
        off += ((size_t)L.m_tiles_s * L.n_chunks_s * ts.TPC * 2 * ts.MT() * 16 / 2 + 63) &
               ~(size_t)63;
        L.bs_off = off;
        off += ((size_t)L.m_tiles_s * ts.MT() + 63) & ~(size_t)63;
      }
      // k = 2u upsamplers (padding u/2): the output-frame kernel's own packing
      const int rows_f = L.kind == L_UPS ? L.C_out * L.s / 2 : 0;
      if (L.kind == L_UPS && h->ups_frames && L.k == 2 * L.s && hfg::ups_rate_ok(L.s) &&
          L.p == L.s / 2 && L.C_in % 16 == 0) {
        // the 32-row tile (3 waves per SIMD) where the 64-row one does not divide the rows
        // (running more stages on it measured slower: two m-tiles stage one window twice)
        const bool small = rows_f % hfg::kUpsCfgs[1].MT() == 0 &&
                           rows_f % hfg::kUpsCfgs[0].MT() != 0;
        const int cfg = small                                 ? 1
                        : rows_f % hfg::kUpsCfgs[0].MT() == 0 ? 0
                                                               : -1;
        if (cfg >= 0) {
          const hfg::UpsCfg& tf = hfg::kUpsCfgs[cfg];
          L.ups_cfg = cfg;
          L.m_tiles_f = rows_f / tf.MT();
          L.wf_off = off;
          // bf16: m-tiles x groups x (class, tap, plane) x rows x 16 ch
          off += ((size_t)L.m_tiles_f * (L.C_in / 16) * 8 * tf.MT() * 16 / 2 + 63) & ~(size_t)63;
          L.bf_off = off;
          off += ((size_t)L.C_out + 63) & ~(size_t)63;
        }
      }
      continue;
    }
    L.prec = 0;
    L.tile = hfg::tile_for_rows(L.M);
    if (!hfg::fp32_conv_supported(L.tile, L.KT, L.dil))
      return fail(HFG_EINVAL, "%s: %d taps at dilation %d span (k-1)*d = %d samples, beyond the "
                  "conv kernels' staging window (max %d)", L.mod.c_str(), L.KT, L.dil,
                  (L.KT - 1) * L.dil, hfg::halo_max(hfg::dispatch_kt(L.KT)));
    const TileCfg& t = kTiles[L.tile];
    L.CK = hfg::ck_for(hfg::dispatch_kt(L.KT), L.tile);
    L.m_tiles = (L.M + t.MT() - 1) / t.MT();
    L.n_chunks = (L.C_in + L.CK - 1) / L.CK;
    L.w_off = off;
    L.w_len = (size_t)L.m_tiles * L.n_chunks * t.MT() * L.CK * L.KT;
    off += (L.w_len + 63) & ~(size_t)63;
    L.b_off = off;
    L.b_len = (size_t)L.m_tiles * t.MT();
    off += (L.b_len + 63) & ~(size_t)63;
  }
  // whole-ResBlock launches (bf16x3 only): every ResBlock of the C in {32, 64} stages, and
  // those of C = 128 whose receptive field costs <= 15% recomputation (k = 3 in V1)
  for (size_t i = 0; i < h->stages.size(); ++i) {
    Stage& st = h->stages[i];
    const int C = st.C;
    st.rbs.assign(c.n_res, RbFused{});
    if (!split_dtype(h->cfg.dtype) || !h->use_fused_rb || (C != 32 && C != 64 && C != 128))
      continue;
    int idx = 0;
    for (int j = 0; j < c.n_res; ++j) {
      RbFused rb;
      rb.kt = c.res_kernels[j];
      // C = 64, k = 3: a 256-column window (5 % more halo recompute than 512) whose small
      // LDS footprint lets two blocks share a CU and overlap their operand rewrites
      const int nwin = C == 128 ? 256 : C == 64 ? (rb.kt == 3 ? 256 : 512) : 512;
      rb.nwin = nwin;
      rb.wm = 1;
      if (c.resblock_type == 1) {
        // ResBlock2 (resblock2_bf16x3): n_dil convs; the first is exact on the whole window
        // (margin rows), so the halo is the radius of the convs after it.  One launch per
        // block, one window per thread block (no split, no persistent grid, no fused conv_post)
        bool ok2 = rb.kt % 2 == 1 && hfg::rb2_supported(C, rb.kt, nwin, rb.wm) &&
                   c.n_dil[j] <= hfg::kRbMaxConv;
        for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
          rb.convs.push_back(st.conv1[idx]);
          if (m > 0) rb.halo += (rb.kt - 1) / 2 * c.dil[j][m];
          if ((rb.kt - 1) / 2 * c.dil[j][m] > hfg::rb_marg(C, nwin)) ok2 = false;
        }
        rb.W = (nwin - 2 * rb.halo) & ~3;
        if (rb.W < nwin / 4) ok2 = false;
        if (C == 128 && (double)nwin / rb.W > 1.15) ok2 = false;
        if (!ok2) continue;
        rb.fused = true;
        rb.w_off = off;
        rb.w_len = (size_t)rb.convs.size() * C * C * rb.kt;
        off += (rb.w_len + 63) & ~(size_t)63;
        rb.b_off = off;
        rb.b_len = rb.convs.size() * (size_t)C;
        off += (rb.b_len + 63) & ~(size_t)63;
        st.rbs[j] = std::move(rb);
        continue;
      }
      bool ok = rb.kt % 2 == 1 && hfg::rb_supported(C, rb.kt, nwin, rb.wm) &&
                2 * c.n_dil[j] <= hfg::kRbMaxConv;
      for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
        rb.convs.push_back(st.conv1[idx]);
        rb.convs.push_back(st.conv2[idx]);
        rb.halo += (rb.kt - 1) / 2 * c.dil[j][m] + (rb.kt - 1) / 2;
        if ((rb.kt - 1) / 2 * c.dil[j][m] > hfg::rb_marg(C, nwin)) ok = false;
      }
      // the first conv of a launch reads its radius of x beyond the window (the LDS margin
      // rows) and is exact on the whole window: the halo is the radius of the convs after it
      rb.halo -= (rb.kt - 1) / 2 * c.dil[j][0];
      // a multiple of 4: block origins t0 = W * blockIdx stay 16-B aligned for the
      // LDS-staged float4 MRF epilogue (which column a block computes does not change
      // its arithmetic: bitwise the same result for any W)
      rb.W = (nwin - 2 * rb.halo) & ~3;
      if (rb.W < nwin / 4) ok = false;
      if (C == 128 && (double)nwin / rb.W > 1.15) ok = false;
      if (!ok) continue;
      rb.fused = true;
      // two launches where that cuts the MFMA work (windows / W, weighted by the convs of
      // each part) by >= 10 %: the extra x write + read costs less than that at C <= 64
      if (h->rb_split && C <= 64 && c.n_dil[j] >= 2) {
        std::vector<int> hd;  // receptive-field radius of each dilation pair
        for (int m = 0; m < c.n_dil[j]; ++m)
          hd.push_back((rb.kt - 1) / 2 * c.dil[j][m] + (rb.kt - 1) / 2);
        // the network's last MRF write may carry the fused conv_post (post_fusable): its
        // launch (the last part) is exact on conv_post's radius 3 more on either side
        const int post = h->fuse_post && i + 1 == h->stages.size() && j == c.n_res - 1 &&
                                 C == 32 && h->conv_post >= 0
                             ? 3 : 0;
        const int w_whole = (nwin - 2 * (rb.halo + post)) & ~3;
        const double whole = w_whole >= nwin / 4 ? (double)nwin / w_whole : 1e9;
        double best = whole;
        for (int m = 1; m < c.n_dil[j]; ++m) {
          int h0 = 0, h1 = 0;
          for (int q = 0; q < m; ++q) h0 += hd[q];
          for (int q = m; q < c.n_dil[j]; ++q) h1 += hd[q];
          h0 -= (rb.kt - 1) / 2 * c.dil[j][0];  // each part's first conv: exact (margins)
          h1 -= (rb.kt - 1) / 2 * c.dil[j][m];
          const int w0 = (nwin - 2 * h0) & ~3, w1 = (nwin - 2 * h1) & ~3;
          const int w1p = (nwin - 2 * (h1 + post)) & ~3;  // the launch as it runs
          if (w0 < nwin / 4 || w1p < nwin / 4) continue;
          const double cost = ((double)m * nwin / w0 + (double)(c.n_dil[j] - m) * nwin / w1p) /
                              c.n_dil[j];
          if (cost < best) {
            best = cost;
            rb.split = 2 * m;
            rb.halo_p[0] = h0;
            rb.halo_p[1] = h1;
            rb.W_p[0] = w0;
            rb.W_p[1] = w1;
          }
        }
        if (best > 0.9 * whole) rb.split = 0;
      }
      rb.w_off = off;
      rb.w_len = (size_t)rb.convs.size() * C * C * rb.kt;  // bf16 hi + lo = one float each
      off += (rb.w_len + 63) & ~(size_t)63;
      rb.b_off = off;
      rb.b_len = rb.convs.size() * (size_t)C;
      off += (rb.b_len + 63) & ~(size_t)63;
      st.rbs[j] = std::move(rb);
    }
  }
  // thin stages (C <= 16, both precisions): one mrf_thin launch per MRF
  for (auto& st : h->stages) {
    const int C = st.C;
    const int nwin = hfg::thin_window(C);
    // (the mrf_thin kernels compute dilation pairs only: ResBlock2 stages run layer by layer)
    if (nwin == 0 || c.n_res > hfg::kThinMaxRes || c.resblock_type == 1) continue;
    int n_conv = 0, halo_max = 0;
    bool ok = true;
    std::vector<int> convs, conv0, halos;
    int idx = 0;
    for (int j = 0; j < c.n_res; ++j) {
      conv0.push_back((int)convs.size());
      int halo = 0;
      for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
        convs.push_back(st.conv1[idx]);
        convs.push_back(st.conv2[idx]);
        const int kr = c.res_kernels[j];
        if ((kr - 1) / 2 * c.dil[j][m] > hfg::kThinMarg) ok = false;
        halo += (kr - 1) / 2 * c.dil[j][m] + (kr - 1) / 2;
      }
      halos.push_back(halo);
      halo_max = std::max(halo_max, halo);
    }
    conv0.push_back((int)convs.size());
    n_conv = (int)convs.size();
    if (n_conv > hfg::kThinMaxConv || nwin - 2 * halo_max < nwin / 4) ok = false;
    if (!ok) continue;
    st.thin = true;
    st.thin_convs = convs;
    st.thin_conv0 = conv0;
    st.thin_halo = halos;
    st.thin_w_off.clear();
    for (int cv : convs) {
      st.thin_w_off.push_back(off);
      off += ((size_t)h->layers[cv].k * C * C + 63) & ~(size_t)63;
    }
    st.thin_b_off = off;
    off += ((size_t)n_conv * C + 63) & ~(size_t)63;
    // bf16x3: the MFMA variant when every conv's zero-padded last k-step stays in the
    // operand margin
    const int tps = 32 / C;
    bool mf = split_dtype(h->cfg.dtype) && C == 16 && hfg::thin_mfma_window(C) > 0 &&
              hfg::thin_mfma_window(C) - 2 * halo_max >= hfg::thin_mfma_window(C) / 4;
    size_t bytes = 0;
    st.thin_m_conv.clear();
    for (int cv : convs) {
      const Layer& Lc = h->layers[cv];
      const int steps = (Lc.k + tps - 1) / tps;
      if (((steps * tps - 1) - (Lc.k - 1) / 2) * Lc.dil > hfg::kThinMarg ||
          steps > hfg::kThinMfmaMaxSteps)
        mf = false;
      st.thin_m_conv.push_back((int)bytes);
      bytes += (size_t)steps * 2048;
    }
    st.thin_mfma = mf;
    if (mf) {
      st.thin_m_off = off;
      st.thin_m_bytes = bytes;
      off += (bytes / 4 + 63) & ~(size_t)63;
    }
  }
  h->packed_host.assign(off, 0.f);
  return HFG_OK;
}

// float -> bf16, round to nearest even (NaN stays NaN)
inline uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// float -> f16 bits, round to nearest even (subnormals kept)
inline uint16_t f2h(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}
inline float h2f(uint16_t u) {
  _Float16 h;
  memcpy(&h, &u, 2);
  return (float)h;
}
// f16x3 exponent of a tensor with max |value| m: m 2^e in [2^14, 2^15), clamped like the
// device's x3_exp (bf16x3_common.h)
int x3_exp_host(float m) {
  if (!(m > 0.f) || !std::isfinite(m)) return 0;
  int x = 0;
  std::frexp(m, &x);
  return std::min(std::max(15 - x, -hfg::kX3ExpMax), hfg::kX3ExpMax);
}
// how one layer's weights are split into the kernels' (hi, lo) planes
struct WSplit {
  int fmt;      // hfg::kFmtBf16 / kFmtF16
  float scale;  // 2^ew (f16)
};
inline WSplit wsplit(const hfg_handle* h, const Layer& L) {
  return WSplit{h->fmt, std::ldexp(1.0f, L.ew)};
}
inline void split_w(float v, const WSplit& ws, uint16_t& hi, uint16_t& lo) {
  if (ws.fmt == hfg::kFmtBf16) {
    hi = f2bf(v);
    lo = f2bf(v - bf2f(hi));
  } else {
    const float a = v * ws.scale;  // exact (power of two)
    hi = f2h(a);
    lo = f2h(a - h2f(hi));
  }
}

// mrf_thin weights: per conv [tap][ci][co] fp32 (the C output channels of one (tap, ci)
// are one scalar load), biases [conv][C]
void pack_thin(hfg_handle* h, const Stage& st) {
  const int C = st.C;
  for (size_t e = 0; e < st.thin_convs.size(); ++e) {
    const Layer& L = h->layers[st.thin_convs[e]];
    const float* w = h->params[L.mod + ".weight"].data.data();  // [C_out][C_in][k]
    float* dst = h->packed_host.data() + st.thin_w_off[e];
    for (int j = 0; j < L.k; ++j)
      for (int ci = 0; ci < C; ++ci)
        for (int co = 0; co < C; ++co)
          dst[((size_t)j * C + ci) * C + co] = w[((size_t)co * C + ci) * L.k + j];
    const float* bsrc = h->params[L.mod + ".bias"].data.data();
    for (int co = 0; co < C; ++co) h->packed_host[st.thin_b_off + e * C + co] = bsrc[co];
  }
  if (!st.thin_mfma) return;
  // mrf_thin_mfma A stream (C = 16): per (conv, k-step) [plane][lane][8], lane l -> row
  // r = l & 15, ci = 8 ((l >> 4) & 1) + e, tap = 2 s + (l >> 5); plane 0 = hi, 1 = lo
  uint16_t* dst = reinterpret_cast<uint16_t*>(h->packed_host.data() + st.thin_m_off);
  const int tps = 32 / C;
  for (size_t e = 0; e < st.thin_convs.size(); ++e) {
    const Layer& L = h->layers[st.thin_convs[e]];
    const WSplit ws = wsplit(h, L);
    const float* w = h->params[L.mod + ".weight"].data.data();  // [C_out][C_in][k]
    const int steps = (L.k + tps - 1) / tps;
    uint16_t* de = dst + st.thin_m_conv[e] / 2;
    for (int s = 0; s < steps; ++s)
      for (int plane = 0; plane < 2; ++plane)
        for (int lane = 0; lane < 64; ++lane)
          for (int el = 0; el < 8; ++el) {
            const int co = lane & 15, qq = lane >> 4;
            const int ci = 8 * (qq & 1) + el, tap = 2 * s + (qq >> 1);
            const float v = tap < L.k ? w[((size_t)co * C + ci) * L.k + tap] : 0.f;
            uint16_t hi, lo;
            split_w(v, ws, hi, lo);
            de[((size_t)(s * 2 + plane) * 64 + lane) * 8 + el] = plane == 0 ? hi : lo;
          }
  }
}

// Fragment order of conv1d_mfma_f32's A operand (see conv_kernels.hip):
//   idx = ((((mt*n_chunks + c)*KT + j)*KK + kk)*WAVES_M + wave_m)*64*WM + lane*WM + wm
//   row = mt*MT + wave_m*32*WM + wm*32 + (lane & 31),  ci = c*CK + 2*kk + (lane >> 5)
// wt(row, ci, j) is the GEMM weight; zero outside [0,M) x [0,C_in).
template <typename F>
void pack_gemm_weights(const Layer& L, F wt, float* dst) {
  const TileCfg& t = kTiles[L.tile];
  const int KK = L.CK / 2;
  size_t idx = 0;
  for (int mt = 0; mt < L.m_tiles; ++mt)
    for (int c = 0; c < L.n_chunks; ++c)
      for (int j = 0; j < L.KT; ++j)
        for (int kk = 0; kk < KK; ++kk)
          for (int wave_m = 0; wave_m < t.WAVES_M; ++wave_m)
            for (int lane = 0; lane < 64; ++lane)
              for (int wm = 0; wm < t.WM; ++wm) {
                const int row = mt * t.MT() + wave_m * 32 * t.WM + wm * 32 + (lane & 31);
                const int ci = c * L.CK + 2 * kk + (lane >> 5);
                dst[idx++] = (row < L.M && ci < L.C_in) ? wt(row, ci, j) : 0.f;
              }
}


// A-fragment order of conv1d_bf16x3 (conv_bf16x3.hip), in bf16 elements:
//   idx = ((((((mt*n_g + g)*n_tg + tg)*TPC + jj)*2 + plane)*WAVES_M + wave_m)*WM + wm)*512
//         + lane*8 + e
//   row = mt*MT + wave_m*32*WM + wm*32 + (lane & 31), ci = g*16 + 8*(lane >> 5) + e,
//   tap = tg*TPC + jj; plane 0 = bf16(w), plane 1 = bf16(w - hi).
template <typename F>
void pack_bf16x3(const Layer& L, F wt, const WSplit& ws, uint16_t* dst) {
  const hfg::Bf16x3Cfg& t = hfg::kBf16x3Tiles[L.tile];
  const int TPC = t.TPC;
  const int n_g = (L.C_in + 15) / 16, n_tg = (L.KT + TPC - 1) / TPC;
  size_t idx = 0;
  for (int mt = 0; mt < L.m_tiles; ++mt)
    for (int g = 0; g < n_g; ++g)
      for (int tg = 0; tg < n_tg; ++tg)
        for (int jj = 0; jj < TPC; ++jj)
          for (int plane = 0; plane < 2; ++plane)
            for (int wave_m = 0; wave_m < t.WAVES_M; ++wave_m)
              for (int wm = 0; wm < t.WM; ++wm)
                for (int lane = 0; lane < 64; ++lane)
                  for (int e = 0; e < 8; ++e) {
                    const int row = mt * t.MT() + wave_m * 32 * t.WM + wm * 32 + (lane & 31);
                    const int ci = g * 16 + 8 * (lane >> 5) + e;
                    const int tap = tg * TPC + jj;
                    float v = 0.f;
                    if (row < L.M && ci < L.C_in && tap < L.KT) v = wt(row, ci, tap);
                    uint16_t hi, lo;
                    split_w(v, ws, hi, lo);
                    dst[idx++] = plane == 0 ? hi : lo;
                  }
}

// A stream of resblock_bf16x3 (resblock_bf16x3.hip), in bf16 elements:
//   idx = (((((wave_m*n_conv + e)*n_g + g)*KT + tap)*2 + plane)*64 + lane)*8 + el
//   row = wave_m*32 + (lane & 31), ci = g*16 + 4*(lane >> 5) + (el & 3) + 8*(el >> 2)
// (the permuted channel order of the kernel's operand planes); plane 0 = bf16(w),
// plane 1 = bf16(w - hi).  Biases [conv][C].
void pack_resblock(hfg_handle* h, const RbFused& rb) {
  uint16_t* dst = reinterpret_cast<uint16_t*>(h->packed_host.data() + rb.w_off);
  float* bdst = h->packed_host.data() + rb.b_off;
  const int n_conv = (int)rb.convs.size();
  const int C = h->layers[rb.convs[0]].C_out;
  const int KT = rb.kt, n_g = C / 16;
  size_t idx = 0;
  for (int wm = 0; wm < C / 32; ++wm)
    for (int e = 0; e < n_conv; ++e) {
      const Layer& L = h->layers[rb.convs[e]];
      const WSplit ws = wsplit(h, L);
      const float* w = h->params[L.mod + ".weight"].data.data();  // [C_out][C_in][k]
      for (int g = 0; g < n_g; ++g)
        for (int tap = 0; tap < KT; ++tap)
          for (int plane = 0; plane < 2; ++plane)
            for (int lane = 0; lane < 64; ++lane)
              for (int el = 0; el < 8; ++el) {
                const int row = wm * 32 + (lane & 31);
                const int ci = g * 16 + 4 * (lane >> 5) + (el & 3) + 8 * (el >> 2);
                const float v = w[((size_t)row * C + ci) * KT + tap];
                uint16_t hi, lo;
                split_w(v, ws, hi, lo);
                dst[idx++] = plane == 0 ? hi : lo;
              }
    }
  for (int e = 0; e < n_conv; ++e) {
    const Layer& L = h->layers[rb.convs[e]];
    const float* bsrc = h->params[L.mod + ".bias"].data.data();
    for (int r = 0; r < C; ++r) bdst[(size_t)e * C + r] = bsrc[r];
  }
}

// A slabs of ups_bf16x3 (ups_bf16x3.hip), in bf16 elements:
//   idx = (((((((mt*n_g + g)*2 + c)*2 + tp)*2 + plane)*WAVES_M + wave_m)*WM + wm)*64 + lane)*8 + e
//   class row rr = mt*MT + wave_m*32*WM + wm*32 + (lane & 31) -> co = rr / h, s' = rr % h
//   (h = u/2), ci = g*16 + 8*(lane >> 5) + e; kernel index (nn.ConvTranspose1d weight
//   [C_in][C_out][k]): class L (c = 0) tap 0 (x[m-1]) s'+h+u, tap 1 (x[m]) s'+h;
//   class R (c = 1) tap 0 (x[m]) s'+u, tap 1 (x[m+1]) s'.  Bias [C_out].
void pack_ups_frames(hfg_handle* h, const Layer& L) {
  const hfg::UpsCfg& t = hfg::kUpsCfgs[L.ups_cfg];
  const float* w = h->params[L.mod + ".weight"].data.data();
  const float* bias = h->params[L.mod + ".bias"].data.data();
  uint16_t* dst = reinterpret_cast<uint16_t*>(h->packed_host.data() + L.wf_off);
  const WSplit ws = wsplit(h, L);
  const int u = L.s, hh = u / 2, k = L.k, cout = L.C_out, n_g = L.C_in / 16;
  size_t idx = 0;
  for (int mt = 0; mt < L.m_tiles_f; ++mt)
    for (int g = 0; g < n_g; ++g)
      for (int c = 0; c < 2; ++c)
        for (int tp = 0; tp < 2; ++tp)
          for (int plane = 0; plane < 2; ++plane)
            for (int wave_m = 0; wave_m < t.WAVES_M; ++wave_m)
              for (int wm = 0; wm < t.WM; ++wm)
                for (int lane = 0; lane < 64; ++lane)
                  for (int e = 0; e < 8; ++e) {
                    const int rr = mt * t.MT() + wave_m * 32 * t.WM + wm * 32 + (lane & 31);
                    const int co = rr / hh, sp = rr % hh;
                    const int ci = g * 16 + 8 * (lane >> 5) + e;
                    const int j = c == 0 ? (tp == 0 ? sp + hh + u : sp + hh) : (tp == 0 ? sp + u : sp);
                    const float v = w[((size_t)ci * cout + co) * k + j];
                    uint16_t hi, lo;
                    split_w(v, ws, hi, lo);
                    dst[idx++] = plane == 0 ? hi : lo;
                  }
  float* bdst = h->packed_host.data() + L.bf_off;
  for (int co = 0; co < cout; ++co) bdst[co] = bias[co];
}

void pack_layer(hfg_handle* h, const Layer& L) {
  const Param& W = h->params[L.mod + ".weight"];
  const Param& Bp = h->params[L.mod + ".bias"];
  float* dst = h->packed_host.data() + L.w_off;
  float* bdst = h->packed_host.data() + L.b_off;
  const float* w = W.data.data();
  if (L.kind == L_POST) {
    std::memcpy(dst, w, sizeof(float) * L.C_in * 7);  // [1][C][7]
    bdst[0] = Bp.data[0];
    return;
  }
  if (L.prec == 1 && (L.kind == L_CONV || L.kind == L_UPS)) {
    // the layer's tile, then (bf16x3 layers with a small-grid packing) the small tile
    for (int pass = 0; pass < (L.tile_s >= 0 ? 2 : 1); ++pass) {
      Layer Lp = L;
      float* wd = dst;
      float* bd = bdst;
      if (pass == 1) {
        Lp.tile = L.tile_s;
        Lp.m_tiles = L.m_tiles_s;
        Lp.n_chunks = L.n_chunks_s;
        Lp.b_len = (size_t)L.m_tiles_s * hfg::kBf16x3Tiles[L.tile_s].MT();
        wd = h->packed_host.data() + L.ws_off;
        bd = h->packed_host.data() + L.bs_off;
      }
      if (L.kind == L_CONV) {
        const int cin = L.C_in, k = L.k;
        pack_bf16x3(Lp, [&](int row, int ci, int j) { return w[((size_t)row * cin + ci) * k + j]; },
                    wsplit(h, L), reinterpret_cast<uint16_t*>(wd));
        for (size_t m = 0; m < Lp.b_len; ++m) bd[m] = m < (size_t)L.M ? Bp.data[m] : 0.f;
      } else {
        const int s = L.s, Q = L.KT, k = L.k, cout = L.C_out;
        pack_bf16x3(Lp,
                    [&](int row, int ci, int jj) {
                      const int co = row / s, r = row % s;
                      const int kidx = r + s * (Q - 1 - jj);
                      return kidx < k ? w[((size_t)ci * cout + co) * k + kidx] : 0.f;
                    },
                    wsplit(h, L), reinterpret_cast<uint16_t*>(wd));
        for (size_t m = 0; m < Lp.b_len; ++m) bd[m] = m < (size_t)L.M ? Bp.data[m / s] : 0.f;
      }
    }
    if (L.ups_cfg >= 0) pack_ups_frames(h, L);
    return;
  }
  if (L.kind == L_CONV) {
    const int cin = L.C_in, k = L.k;
    // nn.Conv1d weight [C_out][C_in][k]
    pack_gemm_weights(L, [&](int row, int ci, int j) { return w[((size_t)row * cin + ci) * k + j]; },
                      dst);
    for (size_t m = 0; m < L.b_len; ++m) bdst[m] = m < (size_t)L.M ? Bp.data[m] : 0.f;
    return;
  }
  // L_UPS: polyphase ConvTranspose1d.  GEMM row m = co*s + r; tap jj reads
  // x[u - (Q-1) + jj], i.e. original kernel index r + s*(Q-1-jj).
  const int s = L.s, Q = L.KT, k = L.k, cout = L.C_out;
  pack_gemm_weights(L,
                    [&](int row, int ci, int jj) {
                      const int co = row / s, r = row % s;
                      const int kidx = r + s * (Q - 1 - jj);
                      if (kidx >= k) return 0.f;
                      // nn.ConvTranspose1d weight [C_in][C_out][k]
                      return w[((size_t)ci * cout + co) * k + kidx];
                    },
                    dst);
  for (size_t m = 0; m < L.b_len; ++m) bdst[m] = m < (size_t)L.M ? Bp.data[m / s] : 0.f;
}

int do_commit(hfg_handle* h) {
  for (auto& key : h->param_order)
    if (!h->params[key].set) return fail(HFG_EAGAIN, "weight '%s' was never set", key.c_str());
  if (h->cfg.dtype == HFG_DTYPE_BF16W) {
    // bf16 weight storage: every conv weight rounded to bf16 (round-to-nearest-even) in
    // place, so every kernel (split planes: lo = 0; fp32 / VALU paths) sees the same
    // bf16-valued weights; biases stay fp32.  Idempotent across commits.
    for (auto& kv : h->params) {
      const std::string& k = kv.first;
      if (k.size() < 7 || k.compare(k.size() - 7, 7, ".weight") != 0) continue;
      for (float& v : kv.second.data) v = bf2f(f2bf(v));
    }
  }
  std::fill(h->packed_host.begin(), h->packed_host.end(), 0.f);
  // f16x3 weight scales: one power of two per layer, from its largest |weight|
  for (auto& L : h->layers) {
    L.ew = 0;
    if (h->fmt != hfg::kFmtF16 || L.kind == L_POST) continue;
    float m = 0.f;
    for (float v : h->params[L.mod + ".weight"].data) m = std::max(m, std::fabs(v));
    L.ew = x3_exp_host(m);
  }
  for (auto& L : h->layers) pack_layer(h, L);
  for (auto& st : h->stages) {
    for (auto& rb : st.rbs)
      if (rb.fused) pack_resblock(h, rb);
    if (st.thin) pack_thin(h, st);
  }
  if (h->device >= 0) {
    DeviceGuard g(h->device);
    if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
    // a previous forward may still read the old weights
    hipError_t se = hipDeviceSynchronize();
    if (se != hipSuccess) return hip_fail(se, "hipDeviceSynchronize(commit)");
    if (h->packed_dev_len < h->packed_host.size()) {
      if (h->packed_dev) (void)hipFree(h->packed_dev);
      h->packed_dev = nullptr;
      h->packed_dev_len = 0;
      hipError_t e = hipMalloc(&h->packed_dev, sizeof(float) * h->packed_host.size());
      if (e != hipSuccess) return fail(HFG_ENOMEM, "hipMalloc(weights): %s", hipGetErrorString(e));
      h->packed_dev_len = h->packed_host.size();
    }
    hipError_t e = hipMemcpy(h->packed_dev, h->packed_host.data(),
                             sizeof(float) * h->packed_host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(weights)");
  }
  h->dirty = false;
  return HFG_OK;
}

// ---- shape bookkeeping ------------------------------------------------------
struct Shapes {
  std::vector<int64_t> L;  // L[0] = T, L[i+1] = length after stage i
  int64_t buf_elems;       // per-buffer elements (all B items)
  int64_t item_elems;      // largest per-item activation (max over stages of C * L)
};

Shapes shapes_for(const hfg_handle* h, int64_t B, int64_t T) {
  Shapes s;
  s.L.push_back(T);
  int64_t mx = (int64_t)h->cfg.c0 * T;
  for (int i = 0; i < h->cfg.n_up; ++i) {
    const int u = h->cfg.up_rates[i], k = h->cfg.up_kernels[i];
    int p = (k - u) / 2;
    if (k - u < 0 && (k - u) % 2 != 0) p -= 1;
    const int64_t lo = (s.L.back() - 1) * u - 2 * p + k;
    s.L.push_back(lo);
    mx = std::max(mx, (int64_t)(h->cfg.c0 >> (i + 1)) * std::max<int64_t>(lo, 0));
  }
  s.item_elems = mx;
  s.buf_elems = ((mx * B + 63) / 64) * 64;
  return s;
}

// 4 activation buffers + the per-stage length table of a ragged batch
size_t lens_table_bytes(const hfg_handle* h, int64_t B) {
  return (((size_t)(h->cfg.n_up + 1) * (size_t)B * sizeof(int32_t)) + 255) & ~(size_t)255;
}
// concurrent ResBlocks for a stage whose grids leave CUs idle: fewer tile-3 blocks (128 rows
// x 256 columns) per conv than HFG_CONC_BLOCKS.  512 (the chip's tile-3 slots) until round 6;
// with the cheaper mrf_combine, 2048 also takes the whole-ResBlock stages of mid-size single-
// stream forwards (same-box sweep, profiles/r06/c1/c1_ab_cb.txt: 4 x 512 frames -3.7 %,
// 32 x 62 -1.6 %, 1 x 4096 -0.8 %, 1 x 8192 and 16 x 256 unchanged; 4096 cost 1 x 8192 +1.2 %)
#ifndef HFG_CONC_BLOCKS
#define HFG_CONC_BLOCKS 2048
#endif
bool stage_conc(const hfg_handle* h, const Stage& st, int64_t B, int64_t L) {
  const int n_res = h->cfg.n_res;
  if (h->rb_conc == 0 || st.thin || n_res < 2 || n_res > hfg::kMrfCombineMax) return false;
  if (h->rb_conc == 1) return true;
  return B * ((L + 255) / 256) * ((st.C + 127) / 128) < HFG_CONC_BLOCKS;
}
bool any_conc(const hfg_handle* h, int64_t B, int64_t T) {
  if (h->mrf_only) return false;
  const Shapes sh = shapes_for(h, B, T);
  for (size_t i = 0; i < h->stages.size(); ++i)
    if (stage_conc(h, h->stages[i], B, sh.L[i + 1])) return true;
  return false;
}
// activation buffers of one forward_impl call: X, R, Tb, MRF, and with concurrent
// ResBlocks an R / Tb / output triple per ResBlock
int n_bufs(const hfg_handle* h, int64_t B, int64_t T, bool conc_ok) {
  return 4 + (conc_ok && any_conc(h, B, T) ? 3 * h->cfg.n_res : 0);
}
// f16x3 scale slots of one forward part: one [B] row of per-item max |value| per producing
// launch (the mel's absmax, conv_pre, every upsampler, layer conv and MRF output), zeroed at
// the start of the forward
int n_slots(const hfg_handle* h) { return (int)h->layers.size() + 2 * h->cfg.n_up + 4; }
size_t slots_bytes(const hfg_handle* h, int64_t B) {
  if (h->fmt != hfg::kFmtF16) return 0;
  return ((size_t)n_slots(h) * (size_t)B * hfg::kAmaxSlotWords * sizeof(uint32_t) + 255) & ~(size_t)255;
}
// workspace of one forward_impl call (one batch half)
size_t ws_part_bytes(const hfg_handle* h, int64_t B, int64_t T, bool conc_ok = false) {
  const size_t n = (size_t)n_bufs(h, B, T, conc_ok) * sizeof(float) *
                       (size_t)shapes_for(h, B, T).buf_elems +
                   lens_table_bytes(h, B) + slots_bytes(h, B);
  return (n + 255) & ~(size_t)255;
}
// small forwards stay on one stream: splitting them doubles an already latency-bound
// launch count (measured: 32 x 62 frames 5.4 -> 5.6 ms split)
bool split_batch(const hfg_handle* h, int64_t B, int64_t T) {
  return h->split >= 2 && B >= 2 && B * T >= hfg_handle::kSplitMinFrames;
}
// workspace of a forward: both halves' when the batch is split over two streams (whose
// ResBlocks then run one after another), else one part with concurrent ResBlocks allowed
size_t ws_bytes_for(const hfg_handle* h, int64_t B, int64_t T) {
  if (!split_batch(h, B, T)) return ws_part_bytes(h, B, T, true);
  const int64_t B1 = (B + 1) / 2;
  return ws_part_bytes(h, B1, T) + ws_part_bytes(h, B - B1, T);
}

hipEvent_t pool_event(hfg_handle* h) {
  if (!h->event_pool.empty()) {
    hipEvent_t e = h->event_pool.back();
    h->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

void recycle_prof(hfg_handle* h) {
  for (auto& r : h->prof) {
    if (r.e0) h->event_pool.push_back(r.e0);
    if (r.e1) h->event_pool.push_back(r.e1);
  }
  h->prof.clear();
}

// f16x3 activation scales of one forward part (bf16x3_common.h): slot rows handed out in
// launch order; base null in the unscaled modes (every take() is then null)
struct Slots {
  uint32_t* base = nullptr;
  int n = 0, next = 0;
  int64_t B = 0;
  uint32_t* take() {
    if (!base) return nullptr;
    if (next >= n) {  // sized by n_slots(): a schedule that needs more is a bug
      overflow = true;
      return nullptr;
    }
    return base + (size_t)(next++) * (size_t)B * hfg::kAmaxSlotWords;
  }
  bool overflow = false;
};

struct Launcher {
  hfg_handle* h;
  hipStream_t stream;
  int part = 0;
  int seq = 0;
  int conc = 1;  // launches of this schedule running side by side (concurrent ResBlocks)
  Slots* sl = nullptr;
  ProfRec* rec = nullptr;
  uint32_t* take() { return sl ? sl->take() : nullptr; }
  void begin(double flop, double bytes) {
    rec = nullptr;
    if (!h->profiling) return;
    ProfRec r{nullptr, flop, bytes, pool_event(h), pool_event(h), h->fwd_count, part, seq++};
    if (r.e0) (void)hipEventRecord(r.e0, stream);
    h->prof.push_back(r);
    rec = &h->prof.back();
  }
  void end(const char* label) {
    if (!rec) return;
    rec->label = label;
    if (rec->e1) (void)hipEventRecord(rec->e1, stream);
  }
};

// Small-grid switch of a bf16x3 layer launch: when the layer's tile leaves most CUs idle
// (fewer than kSmallGridBlocks blocks), run the small tile on its own packing.  Bitwise
// the same result (kernels.h, tile 4).  Updates p's weights / chunks; returns the tile.
int pick_tile(const hfg_handle* h, const Layer& L, hfg::ConvParams& p, int64_t n_cols, int64_t B,
              int conc, int& n_tiles, int& m_tiles) {
  int tile = L.tile;
  m_tiles = L.m_tiles;
  if (L.prec != 1 || L.tile_s < 0 || h->small_tile == 0)
    return tile;
  // conc: the grids of that many concurrent launches share the chip
  const bool small =
      h->small_tile == 1 || (int64_t)n_tiles * m_tiles * B * conc < hfg::kSmallGridBlocks;
  if (!small) return tile;
  tile = L.tile_s;
  m_tiles = L.m_tiles_s;
  n_tiles = (int)((n_cols + hfg::kBf16x3Tiles[tile].NTILE() - 1) / hfg::kBf16x3Tiles[tile].NTILE());
  p.w = h->packed_dev + L.ws_off;
  p.bias = h->packed_dev + L.bs_off;
  p.n_chunks = L.n_chunks_s;
  return tile;
}

// One conv-layer launch (regular Conv1d).
// ain / aout: f16x3 scale slots of the input (its producer's) and of this launch's output
int run_conv(hfg_handle* h, Launcher& ln, const Layer& L, const float* x, int64_t B, int64_t Lt,
             float* y, bool act_in, bool act_out, const float* res, float* mrf, int mrf_mode,
             float mrf_div, const int32_t* lens, const uint32_t* ain, uint32_t* aout,
             bool x_btc = false) {
  ConvParams p{};
  p.x = x;
  p.x_bs = (int64_t)L.C_in * Lt;
  p.x_cs = x_btc ? 1 : Lt;          // [B][T][C] (acoustic-model layout) or [B][C][T]
  p.x_ts = x_btc ? L.C_in : 1;
  p.C_in = L.C_in;
  p.L_in = (int)Lt;
  p.len_in = lens;
  p.len_out = lens;
  p.w = h->packed_dev + L.w_off;
  p.bias = h->packed_dev + L.b_off;
  p.y = y;
  p.y_bs = (int64_t)L.C_out * Lt;
  p.M = L.M;
  p.N = (int)Lt;
  p.off = -L.pad;
  p.dil = L.dil;
  p.kt = L.KT;
  p.act_in = act_in;
  p.act_out = act_out;
  p.res = res;
  p.mrf = mrf;
  p.mrf_mode = mrf_mode;
  p.mrf_div = mrf_div;
  p.n_chunks = L.n_chunks;
  p.dbg = h->dbg_flags;
  p.epi_lds = 1;
  p.amax_in = ain;
  p.amax_out = aout;
  p.ew = L.ew;
  const int ntile = L.prec == 1 ? hfg::kBf16x3Tiles[L.tile].NTILE() : kTiles[L.tile].NTILE();
  int n_tiles = (int)((Lt + ntile - 1) / ntile), m_tiles = L.m_tiles;
  const int tile = pick_tile(h, L, p, Lt, B, ln.conc, n_tiles, m_tiles);
  const double flop = 2.0 * L.C_out * L.C_in * L.k * (double)Lt * B;
  double bytes = 4.0 * B * Lt * (L.C_in + L.C_out) + 4.0 * L.C_out * L.C_in * L.k;
  if (res) bytes += 4.0 * B * Lt * L.C_out;
  if (mrf && (mrf_mode & 1)) bytes += 4.0 * B * Lt * L.C_out;
  const char* name = nullptr;
  ln.begin(flop, bytes);
  hipError_t e = L.prec == 1
                     ? hfg::launch_conv_bf16x3(tile, L.KT, false, h->fmt, h->np, p, n_tiles, m_tiles,
                                               (int)B, ln.stream, &name)
                     : hfg::launch_conv((TileId)L.tile, L.KT, false, p, n_tiles, L.m_tiles,
                                        (int)B, ln.stream, &name);
  ln.end(name);
  if (e != hipSuccess) return fail(HFG_EIO, "launch %s: %s", L.mod.c_str(), hipGetErrorString(e));
  return HFG_OK;
}

// slope of the leaky_relu in front of conv_post: the reference's 0.1 (models/hifigan.py:254)
// unless the config names another (the public release's F.leaky_relu(x) default, 0.01)
inline float post_slope_of(const hfg_handle* h) {
  return h->cfg.post_slope ? h->cfg.post_slope : hfg::kLReluSlope;
}

struct PostFuse {
  const float* w;  // conv_post weight [C][7], bias [1] (packed fp32)
  const float* b;
  float* wav;      // [B][L]
  float slope;     // of the leaky_relu in front of conv_post (post_slope_of)
};

// One whole ResBlock (all dilations) + its MRF contribution in one launch.
// A split ResBlock (rb.split) runs as two launches through `scratch` (B*C*L floats): convs
// [0, split) write x after their dilation pairs (MRF-epilogue mode 0: a plain store), convs
// [split, n) read it back and do the MRF epilogue.  fp32 round trip: bitwise the same x.
// post: conv_post + tanh fused into the last launch (C = 32, the network's last MRF write).
int run_resblock(hfg_handle* h, Launcher& ln, const RbFused& rb, const float* x, int64_t B,
                 int64_t Lt, float* mrf, int mrf_mode, float mrf_div, const int32_t* lens,
                 float* scratch, uint32_t* aout, const PostFuse* post = nullptr) {
  const Layer& L0 = h->layers[rb.convs[0]];
  const int C = L0.C_out;
  const int n_all = (int)rb.convs.size();
  const int n_part = rb.split && scratch ? 2 : 1;
  for (int part = 0; part < n_part; ++part) {
    const int c0 = n_part == 1 ? 0 : (part == 0 ? 0 : rb.split);
    const int c1 = n_part == 1 ? n_all : (part == 0 ? rb.split : n_all);
    const bool last = part == n_part - 1;
    hfg::RbParams p{};
    p.x = part == 0 ? x : scratch;
    p.bs = (int64_t)C * Lt;
    p.L = (int)Lt;
    p.len = lens;
    p.w = reinterpret_cast<const __bf16*>(h->packed_dev + rb.w_off);
    p.w_bytes = (int)(rb.w_len * sizeof(float));
    p.bias = h->packed_dev + rb.b_off + (size_t)c0 * C;
    p.n_conv = c1 - c0;
    p.conv0 = c0;
    p.n_conv_stream = n_all;
    double flop = 0.0;
    for (int e = c0; e < c1; ++e) {
      const Layer& L = h->layers[rb.convs[e]];
      p.dil[e - c0] = L.dil;
      p.ew[e - c0] = L.ew;
      flop += 2.0 * L.C_out * L.C_in * L.k * (double)Lt * B;
    }
    p.halo = n_part == 1 ? rb.halo : rb.halo_p[part];
    p.W = n_part == 1 ? rb.W : rb.W_p[part];
    p.mrf = last ? mrf : scratch;
    p.mrf_mode = last ? mrf_mode : 0;
    p.mrf_div = mrf_div;
    p.mrf_rcp = hfg::fast_div_ok(mrf_div) ? 1.0f / mrf_div : 0.0f;
    p.amax_out = last ? aout : nullptr;
    p.dbg = h->dbg_flags;
    // resident blocks per CU from the LDS footprint
    const int per_cu = hfg::rb_lds_bytes(C, rb.nwin, n_all) <= 80 * 1024 ? 2 : 1;
    // a persistent grid of the resident blocks (each window's x load overlaps the previous
    // window's MRF round trip; launch_resblock_bf16x3 runs it where a persistent variant is
    // built, C = 64 with the 512-column window).  HFG_RB_PERSIST: 0 off, 1 one block per CU
    // of the half-batch stream's share (n_CU / halves), 2 one per CU
    const bool rb2 = h->cfg.resblock_type == 1;  // resblock2_bf16x3: one window per block
    if (h->rb_persist && per_cu == 1 && !(last && post) && !rb2)
      p.persist = std::max(1, h->n_cu / (h->rb_persist == 1 ? h->halves : 1));
    double bytes =
        4.0 * B * Lt * C * ((last && (mrf_mode & 1)) ? 3 : 2) + 4.0 * (double)rb.w_len;
    if (last && post) {
      // the stage output is exact on the centre plus conv_post's radius on either side
      p.halo += 3;
      p.W = (rb.nwin - 2 * p.halo) & ~3;
      p.post_w = post->w;
      p.post_b = post->b;
      p.post_slope = post->slope;
      p.wav = post->wav;
      p.amax_out = nullptr;  // no consumer of the stage output's scale
      bytes -= 4.0 * B * Lt * (C - 1);
    }
    const char* name = nullptr;
    ln.begin(flop, bytes);
    hipError_t e =
        rb2 ? hfg::launch_resblock2_bf16x3(C, rb.nwin, rb.wm, rb.kt, h->fmt, h->np, p, (int)B,
                                           ln.stream, &name)
            : hfg::launch_resblock_bf16x3(C, rb.nwin, rb.wm, rb.kt, h->fmt, h->np, p, (int)B,
                                          ln.stream, &name);
    ln.end(name);
    if (e != hipSuccess)
      return fail(HFG_EIO, "launch resblock %s: %s", L0.mod.c_str(), hipGetErrorString(e));
  }
  return HFG_OK;
}

int run_ups(hfg_handle* h, Launcher& ln, const Layer& L, const float* x, int64_t B, int64_t Lin,
            int64_t Lout, float* y, const int32_t* len_in, const int32_t* len_out,
            const uint32_t* ain, uint32_t* aout) {
  const double flop = 2.0 * L.C_in * L.C_out * L.k * (double)Lin * B;
  const double bytes = 4.0 * B * (L.C_in * Lin + L.C_out * Lout) + 4.0 * L.C_in * L.C_out * L.k;
  if (L.ups_cfg >= 0 && h->ups_frames && Lin % 4 == 0 && Lout == Lin * L.s) {
    // output-frame kernel, unless its grid would leave most CUs idle (then the polyphase
    // kernel's small-grid tile): bitwise the same result either way
    const int cfg = L.ups_cfg;
    const hfg::UpsCfg& t = hfg::kUpsCfgs[cfg];
    const int n_tiles = (int)((Lin + t.NTILE() - 1) / t.NTILE());
    if (h->ups_frames == 2 ||
        (int64_t)L.m_tiles_f * n_tiles * B * ln.conc >= hfg::kSmallGridBlocks) {
      hfg::UpsParams q{};
      q.x = x;
      q.x_bs = (int64_t)L.C_in * Lin;
      q.C_in = L.C_in;
      q.L = (int)Lin;
      q.T = (int)Lin;
      q.len_in = len_in;
      q.w = reinterpret_cast<const __bf16*>(h->packed_dev + L.wf_off);
      q.bias = h->packed_dev + L.bf_off;
      q.y = y;
      q.y_bs = (int64_t)L.C_out * Lout;
      q.C_out = L.C_out;
      q.L_out = (int)Lout;
      q.u = L.s;
      q.m_tiles = L.m_tiles_f;
      q.n_tiles = n_tiles;
      q.batch = (int)B;
      q.amax_in = ain;
      q.amax_out = aout;
      q.ew = L.ew;
      q.dbg = h->dbg_flags;
      const char* name = nullptr;
      ln.begin(flop, bytes);
      hipError_t e = hfg::launch_ups_bf16x3(cfg, h->fmt, h->np, q, ln.stream, &name);
      ln.end(name);
      if (e != hipSuccess)
        return fail(HFG_EIO, "launch %s: %s", L.mod.c_str(), hipGetErrorString(e));
      return HFG_OK;
    }
  }
  ConvParams p{};
  p.x = x;
  p.x_bs = (int64_t)L.C_in * Lin;
  p.x_cs = Lin;
  p.x_ts = 1;
  p.C_in = L.C_in;
  p.L_in = (int)Lin;
  p.len_in = len_in;
  p.len_out = len_out;
  p.w = h->packed_dev + L.w_off;
  p.bias = h->packed_dev + L.b_off;
  p.y = y;
  p.y_bs = (int64_t)L.C_out * Lout;
  p.M = L.M;
  // columns u: t_out + p = s*u + r  for t_out in [0, Lout)
  p.N = (int)((Lout - 1 + L.p) / L.s + 1);
  p.off = -(L.KT - 1);
  p.dil = 1;
  p.kt = L.KT;
  p.act_in = 1;  // F.leaky_relu before every upsample, models/hifigan.py:244
  p.act_out = 0;
  p.ups_s = L.s;
  p.ups_p = L.p;
  p.ups_swz = 1;
  p.L_out = (int)Lout;
  p.n_chunks = L.n_chunks;
  p.amax_in = ain;
  p.amax_out = aout;
  p.ew = L.ew;
  p.dbg = h->dbg_flags;
  const int ntile = L.prec == 1 ? hfg::kBf16x3Tiles[L.tile].NTILE() : kTiles[L.tile].NTILE();
  int n_tiles = (p.N + ntile - 1) / ntile, m_tiles = L.m_tiles;
  const int tile = pick_tile(h, L, p, p.N, B, ln.conc, n_tiles, m_tiles);
  const char* name = nullptr;
  ln.begin(flop, bytes);
  hipError_t e = L.prec == 1
                     ? hfg::launch_conv_bf16x3(tile, L.KT, true, h->fmt, h->np, p, n_tiles, m_tiles,
                                               (int)B, ln.stream, &name)
                     : hfg::launch_conv((TileId)L.tile, L.KT, true, p, n_tiles, L.m_tiles, (int)B,
                                        ln.stream, &name);
  ln.end(name);
  if (e != hipSuccess) return fail(HFG_EIO, "launch %s: %s", L.mod.c_str(), hipGetErrorString(e));
  return HFG_OK;
}

// A thin stage's whole MRF (or ResBlock only_j alone) in one mrf_thin launch.
int run_thin(hfg_handle* h, Launcher& ln, const Stage& st, const float* X, int64_t B, int64_t Lt,
             float* out, const int32_t* lens, int only_j, uint32_t* aout) {
  const hfg_config& c = h->cfg;
  const int C = st.C;
  hfg::ThinParams p{};
  p.x = X;
  p.bs = (int64_t)C * Lt;
  p.L = (int)Lt;
  p.len = lens;
  p.w = h->packed_dev;
  p.bias = h->packed_dev + st.thin_b_off;
  const int j0 = only_j >= 0 ? only_j : 0, j1 = only_j >= 0 ? only_j + 1 : c.n_res;
  p.n_res = j1 - j0;
  const int cv_base = st.thin_conv0[j0];
  double flop = 0.0, wbytes = 0.0;
  int halo = 0;
  for (int j = j0; j < j1; ++j) {
    p.rb_conv0[j - j0] = st.thin_conv0[j] - cv_base;
    halo = std::max(halo, st.thin_halo[j]);
  }
  p.rb_conv0[p.n_res] = st.thin_conv0[j1] - cv_base;
  for (int e = st.thin_conv0[j0]; e < st.thin_conv0[j1]; ++e) {
    const Layer& L = h->layers[st.thin_convs[e]];
    const int q = e - cv_base;
    p.kt[q] = L.k;
    p.dil[q] = L.dil;
    p.ew[q] = L.ew;
    p.w_off[q] = (int)st.thin_w_off[e];
    flop += 2.0 * C * C * L.k * (double)Lt * B;
    wbytes += 4.0 * C * C * L.k;
  }
  // the kernel indexes biases as [conv][C] from this launch's first conv
  p.bias = h->packed_dev + st.thin_b_off + (size_t)cv_base * C;
  p.halo = halo;
  p.W = (st.thin_mfma ? hfg::thin_mfma_window(C) : hfg::thin_window(C)) - 2 * halo;
  p.y = out;
  p.div = (float)p.n_res;
  p.amax_out = aout;
  if (st.thin_mfma) {
    const int base = st.thin_m_conv[cv_base];
    p.wm = reinterpret_cast<const __bf16*>(h->packed_dev + st.thin_m_off) + base / 2;
    p.wm_bytes = (int)st.thin_m_bytes - base;
    for (int e = st.thin_conv0[j0]; e < st.thin_conv0[j1]; ++e)
      p.wm_off[e - cv_base] = st.thin_m_conv[e] - base;
  }
  const double bytes = 8.0 * B * Lt * C + wbytes;  // x once, y once, weights once
  const char* name = nullptr;
  ln.begin(flop, bytes);
  hipError_t e = st.thin_mfma ? hfg::launch_mrf_thin_mfma(C, h->fmt, h->np, p, (int)B, ln.stream, &name)
                               : hfg::launch_mrf_thin(C, p, (int)B, ln.stream, &name);
  ln.end(name);
  if (e != hipSuccess) return fail(HFG_EIO, "launch mrf_thin (C=%d): %s", C, hipGetErrorString(e));
  return HFG_OK;
}

// ResBlock j of stage st (ResBlock.forward, models/hifigan.py:72-86) on X, its result
// combined into out by the MRF epilogue mode (bit0 add, bit1 divide by n_res); idx = index
// of its first dilation in st.conv1 / st.conv2.  R, Tb: scratch of the layer-per-launch path.
// f16x3: ax = scale slot of X; aout = slot of out (committed by the write that completes it)
int run_one_rb(hfg_handle* h, Launcher& ln, const Stage& st, int j, int idx, const float* X,
               int64_t B, int64_t L, float* R, float* Tb, float* out, int mode,
               const int32_t* lens, const uint32_t* ax, uint32_t* aout,
               const PostFuse* post = nullptr) {
  const hfg_config& c = h->cfg;
  if (st.rbs[j].fused)
    return run_resblock(h, ln, st.rbs[j], X, B, L, out, mode, (float)c.n_res, lens, Tb, aout,
                        post);
  int rc;
  const uint32_t* asrc = ax;
  if (c.resblock_type == 1) {
    // ResBlock2, one launch per dilation: x = x + conv_m(lrelu(x)).  The conv reads a
    // neighbourhood of x, so it writes the other of R / Tb; the last one carries the MRF epilogue
    const float* src = X;
    for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
      const Layer& Lm = h->layers[st.conv1[idx]];
      if (m < c.n_dil[j] - 1) {
        float* dst = (m & 1) ? Tb : R;
        uint32_t* ar = ln.take();
        rc = run_conv(h, ln, Lm, src, B, L, dst, true, false, src, nullptr, 0, 1.f, lens, asrc, ar);
        src = dst;
        asrc = ar;
      } else {
        rc = run_conv(h, ln, Lm, src, B, L, nullptr, true, false, src, out, mode, (float)c.n_res,
                      lens, asrc, aout);
      }
      if (rc) return rc;
    }
    return HFG_OK;
  }
  for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
    const float* src = (m == 0) ? X : R;
    const Layer& L1 = h->layers[st.conv1[idx]];
    const Layer& L2 = h->layers[st.conv2[idx]];
    // xt = lrelu(conv1(lrelu(x)))
    uint32_t* at = ln.take();
    rc = run_conv(h, ln, L1, src, B, L, Tb, true, true, nullptr, nullptr, 0, 1.f, lens, asrc, at);
    if (rc) return rc;
    if (m < c.n_dil[j] - 1) {
      // x = x + conv2(xt)
      uint32_t* ar = ln.take();
      rc = run_conv(h, ln, L2, Tb, B, L, R, false, false, src, nullptr, 0, 1.f, lens, at, ar);
      asrc = ar;
    } else {
      rc = run_conv(h, ln, L2, Tb, B, L, nullptr, false, false, src, out, mode, (float)c.n_res,
                    lens, at, aout);
    }
    if (rc) return rc;
  }
  return HFG_OK;
}

// Scratch of the concurrent-ResBlock schedule: per ResBlock its R / Tb and its output.
struct RbConc {
  float* R[HFG_MAX_RES];
  float* Tb[HFG_MAX_RES];
  float* O[HFG_MAX_RES];
};

// Aux streams of one batch part (created on first use; hipStreamNonBlocking)
int rb_streams(hfg_handle* h, int part) {
  for (int j = 0; j < h->cfg.n_res - 1; ++j)
    if (!h->rb_aux[part][j]) {
      hipError_t e = hipStreamCreateWithFlags(&h->rb_aux[part][j], hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&h->rb_join[part][j], hipEventDisableTiming);
      if (e != hipSuccess) return hip_fail(e, "create ResBlock stream");
    }
  if (!h->rb_fork[part]) {
    hipError_t e = hipEventCreateWithFlags(&h->rb_fork[part], hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(e, "create ResBlock fork event");
  }
  return HFG_OK;
}

// MRF of stage st (models/hifigan.py:116-131) on X [B][C][L]: out = mean_j ResBlock_j(X)
// (ResBlock.forward :72-86), or out = ResBlock_only_j(X) alone when only_j >= 0.  R and Tb
// are B*C*L-float scratch buffers of the layer-per-launch ResBlocks; out must not alias X.
// With conc set, the ResBlocks run concurrently (ResBlock j > 0 on aux stream j-1 of this
// batch part), each into its own output, and one combine launch forms the mean in the
// sequential schedule's order — bitwise the same result, for grids that leave CUs idle.
// ax: f16x3 scale slot of X; aout: slot of out (the MRF mean, or ResBlock only_j's output)
int run_mrf(hfg_handle* h, Launcher& ln, const Stage& st, const float* X, int64_t B, int64_t L,
            float* R, float* Tb, float* out, const int32_t* lens, int only_j,
            const uint32_t* ax, uint32_t* aout, const RbConc* conc = nullptr,
            const PostFuse* post = nullptr) {
  const hfg_config& c = h->cfg;
  if (st.thin) return run_thin(h, ln, st, X, B, L, out, lens, only_j, aout);
  int rc;
  if (conc && only_j < 0 && c.n_res > 1) {
    if ((rc = rb_streams(h, ln.part))) return rc;
    hipError_t e = hipEventRecord(h->rb_fork[ln.part], ln.stream);
    for (int j = 1; j < c.n_res && e == hipSuccess; ++j)
      e = hipStreamWaitEvent(h->rb_aux[ln.part][j - 1], h->rb_fork[ln.part], 0);
    if (e != hipSuccess) return hip_fail(e, "ResBlock fork");
    // the ResBlock with the most work (largest kernel-size sum over its dilations) stays on
    // the caller's stream: the aux streams start only after the fork event's cross-queue
    // signal (~10-20 us after the producing launch ends) and the join waits on theirs, so
    // the chain that finishes last should be the one that pays neither (round 6, C1 traces)
    int j_main = 0;
    for (int j = 1; j < c.n_res; ++j)
      if (c.res_kernels[j] * c.n_dil[j] > c.res_kernels[j_main] * c.n_dil[j_main]) j_main = j;
    int idx = 0;
    for (int j = 0, aux = 0; j < c.n_res; ++j) {
      Launcher lj{h, j == j_main ? ln.stream : h->rb_aux[ln.part][aux++], ln.part, ln.seq,
                  c.n_res, ln.sl};
      rc = run_one_rb(h, lj, st, j, idx, X, B, L, conc->R[j], conc->Tb[j], conc->O[j], 0, lens,
                      ax, nullptr);
      if (rc) return rc;
      ln.seq = lj.seq;
      idx += c.n_dil[j];
    }
    for (int j = 1; j < c.n_res && e == hipSuccess; ++j) {
      e = hipEventRecord(h->rb_join[ln.part][j - 1], h->rb_aux[ln.part][j - 1]);
      if (e == hipSuccess) e = hipStreamWaitEvent(ln.stream, h->rb_join[ln.part][j - 1], 0);
    }
    if (e != hipSuccess) return hip_fail(e, "ResBlock join");
    hfg::MrfCombineArgs a{};
    for (int j = 0; j < c.n_res; ++j) a.o[j] = conc->O[j];
    a.n = c.n_res;
    a.C = st.C;
    a.L = (int)L;
    a.len = lens;
    a.y = out;
    a.div = (float)c.n_res;
    a.amax_out = aout;
    ln.begin(0.0, 4.0 * B * L * st.C * (c.n_res + 1));
    e = hfg::launch_mrf_combine(a, (int)B, ln.stream);
    ln.end("mrf_combine");
    if (e != hipSuccess) return hip_fail(e, "launch mrf_combine");
    return HFG_OK;
  }
  int idx = 0;
  for (int j = 0; j < c.n_res; ++j) {
    if (only_j >= 0 && j != only_j) {
      idx += c.n_dil[j];
      continue;
    }
    const int mode = only_j >= 0 ? 0 : ((j > 0 ? 1 : 0) | (j == c.n_res - 1 ? 2 : 0));
    // the write that completes out: the last ResBlock's (the divide), or only_j's
    rc = run_one_rb(h, ln, st, j, idx, X, B, L, R, Tb, out, mode, lens, ax,
                    (only_j >= 0 || (mode & 2)) ? aout : nullptr,
                    only_j < 0 && j == c.n_res - 1 ? post : nullptr);
    if (rc) return rc;
    idx += c.n_dil[j];
  }
  return HFG_OK;
}

// conv_post fused into the last MRF's last ResBlock launch (resblock_bf16x3 conv_post_tail):
// C = 32 on the one-launch-per-ResBlock schedule, L % 4 == 0, no inspection taps (they read
// the stage output, which that launch does not store)
bool post_fusable(const hfg_handle* h, const Stage& st, int64_t L, bool conc_st,
                  float* const* taps) {
  const hfg_config& c = h->cfg;
  if (!h->fuse_post || h->conv_post < 0 || taps || conc_st || st.thin || st.C != 32 ||
      L % 4 != 0 || h->layers[h->conv_post].C_in != 32 || c.resblock_type == 1)
    return false;
  const RbFused& rb = st.rbs[c.n_res - 1];
  if (!rb.fused || rb.nwin != 512 || rb.wm != 1) return false;
  const int halo = (rb.split ? rb.halo_p[1] : rb.halo) + 3;
  return halo >= 4 && ((rb.nwin - 2 * halo) & ~3) >= rb.nwin / 4;
}

// taps (inspection, hfg_forward_taps): taps[0] <- conv_pre output, taps[1 + 2i] <- ups[i]
// output, taps[2 + 2i] <- mrfs[i] output (models/hifigan.py:238-251); NULL entries skipped.
int forward_impl(hfg_handle* h, const float* mel, int64_t B, int64_t T, const hfg_forward_opts* o,
                 float* wav, int64_t out_len, void* ws, size_t ws_len, hipStream_t stream,
                 int part = 0, float* const* taps = nullptr, bool conc_ok = false) {
  if (!mel || !wav) return fail(HFG_EINVAL, "mel / wav pointer is NULL");
  const bool btc = o && o->mel_layout == HFG_MEL_BTC;
  if (o && o->mel_layout != HFG_MEL_BCT && o->mel_layout != HFG_MEL_BTC)
    return fail(HFG_EINVAL, "unknown mel_layout %d", o->mel_layout);
  const int32_t* user_lens = o ? o->lengths : nullptr;
  if (B <= 0 || T <= 0) return fail(HFG_EINVAL, "B and T must be > 0 (got %lld, %lld)",
                                    (long long)B, (long long)T);
  const Shapes sh = shapes_for(h, B, T);
  for (auto l : sh.L)
    if (l <= 0) return fail(HFG_EINVAL, "T=%lld gives an empty stage", (long long)T);
  if (sh.L.back() != out_len)
    return fail(HFG_EINVAL, "out_len %lld != expected %lld", (long long)out_len,
                (long long)sh.L.back());
  // the kernels address one utterance's activations with 32-bit byte offsets from a
  // per-item base, through buffer descriptors of num_records 0xFFFFFFFF.  The hardware
  // drops a dword whose END passes num_records, so a 4 GiB item would lose its last
  // float: an item holds fewer than 2^30 fp32 elements (V1: T <= 131071 frames)
  if (sh.item_elems >= ((int64_t)1 << 30))
    return fail(HFG_EINVAL, "per-item activation of %lld elements reaches 2^30 (T too long)",
                (long long)sh.item_elems);
  if (ws_len < ws_part_bytes(h, B, T, conc_ok)) return fail(HFG_EINVAL, "workspace too small");
  const int nb = n_bufs(h, B, T, conc_ok);
  float* buf[4 + 3 * HFG_MAX_RES];
  for (int i = 0; i < nb; ++i) buf[i] = reinterpret_cast<float*>(ws) + (size_t)i * sh.buf_elems;
  RbConc conc{};
  for (int j = 0; nb > 4 && j < h->cfg.n_res; ++j) {
    conc.R[j] = buf[4 + 3 * j];
    conc.Tb[j] = buf[5 + 3 * j];
    conc.O[j] = buf[6 + 3 * j];
  }
  float* X = buf[0];    // upsampled stage input
  float* R = buf[1];    // running ResBlock state (also conv_pre output)
  float* Tb = buf[2];   // conv1 output
  float* MRF = buf[3];  // MRF accumulator
  Slots sl;
  Launcher ln{h, stream, part};
  ln.sl = &sl;
  const hfg_config& c = h->cfg;
  int rc;
  if (h->fmt == hfg::kFmtF16) {
    // after the activation buffers and the length table (ws_part_bytes)
    sl.base = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) +
                                          (size_t)nb * sh.buf_elems * sizeof(float) +
                                          lens_table_bytes(h, B));
    sl.n = n_slots(h);
    sl.B = B;
    hipError_t e = hipMemsetAsync(sl.base, 0, slots_bytes(h, B), stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(scale slots)");
  }
  // ragged batch: per-stage valid lengths, computed on the device from lengths[B]
  const int32_t* lt = nullptr;  // lt + s*B = lengths after s upsample stages
  if (user_lens) {
    int32_t* table = reinterpret_cast<int32_t*>(reinterpret_cast<float*>(ws) +
                                                (size_t)nb * sh.buf_elems);
    hfg::StageLenParams sp{};
    sp.n_up = c.n_up;
    sp.T = (int)T;
    for (int i = 0; i < c.n_up; ++i) {
      sp.up_rates[i] = c.up_rates[i];
      sp.up_kernels[i] = c.up_kernels[i];
    }
    hipError_t e = hfg::launch_stage_lengths(user_lens, (int)B, sp, table, stream);
    if (e != hipSuccess) return fail(HFG_EIO, "launch stage_lengths: %s", hipGetErrorString(e));
    lt = table;
  }
  auto lens_at = [&](int s) { return lt ? lt + (size_t)s * B : nullptr; };
  auto tap = [&](int k, const float* src, int64_t n) -> int {
    if (!taps || !taps[k]) return HFG_OK;
    hipError_t e = hipMemcpyAsync(taps[k], src, sizeof(float) * (size_t)n,
                                  hipMemcpyDeviceToDevice, stream);
    return e == hipSuccess ? HFG_OK : hip_fail(e, "hipMemcpyAsync(tap)");
  };
  // f16x3: the mel's per-item max |value| (no kernel produced it)
  uint32_t* a_mel = ln.take();
  if (a_mel) {
    ln.begin(0.0, 4.0 * B * c.n_mels * T);
    hipError_t e = hfg::launch_absmax(mel, (int64_t)c.n_mels * T, btc ? 1 : T, btc ? c.n_mels : 1,
                                      c.n_mels, (int)T, lens_at(0), (int)B, a_mel, stream);
    ln.end("absmax");
    if (e != hipSuccess) return fail(HFG_EIO, "launch absmax: %s", hipGetErrorString(e));
  }
  // conv_pre  (models/hifigan.py:238)
  uint32_t* a_cur = ln.take();
  rc = run_conv(h, ln, h->layers[h->conv_pre], mel, B, T, R, false, false, nullptr, nullptr, 0,
                1.f, lens_at(0), a_mel, a_cur, btc);
  if (rc) return rc;
  if ((rc = tap(0, R, B * c.c0 * T))) return rc;
  const float* cur = R;
  for (int i = 0; i < c.n_up; ++i) {
    const Stage& st = h->stages[i];
    const int64_t Lin = sh.L[i], L = sh.L[i + 1];
    // lrelu -> ups[i]  (models/hifigan.py:244-245)
    uint32_t* a_x = ln.take();
    rc = run_ups(h, ln, h->layers[st.conv_ups], cur, B, Lin, L, X, lens_at(i), lens_at(i + 1),
                 a_cur, a_x);
    if (rc) return rc;
    if ((rc = tap(1 + 2 * i, X, B * st.C * L))) return rc;
    // MRF (models/hifigan.py:116-131) of ResBlocks (:72-86)
    a_cur = ln.take();
    const bool conc_st = nb > 4 && stage_conc(h, st, B, L);
    if (i == c.n_up - 1 && post_fusable(h, st, L, conc_st, taps)) {
      // the last ResBlock's launch also runs lrelu -> conv_post -> tanh (models/hifigan.py:
      // 254-256); windows past an item's length write nothing: zero the wav first
      if (user_lens) {
        hipError_t e = hipMemsetAsync(wav, 0, sizeof(float) * (size_t)(B * L), stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(wav)");
      }
      const Layer& Lp = h->layers[h->conv_post];
      const PostFuse pf{h->packed_dev + Lp.w_off, h->packed_dev + Lp.b_off, wav,
                        post_slope_of(h)};
      rc = run_mrf(h, ln, st, X, B, L, R, Tb, MRF, lens_at(i + 1), -1, a_x, a_cur, nullptr, &pf);
      if (rc) return rc;
      if (sl.overflow) return fail(HFG_EIO, "internal: f16x3 scale slots exhausted");
      return HFG_OK;
    }
    rc = run_mrf(h, ln, st, X, B, L, R, Tb, MRF, lens_at(i + 1), -1, a_x, a_cur,
                 conc_st ? &conc : nullptr);
    if (rc) return rc;
    if ((rc = tap(2 + 2 * i, MRF, B * st.C * L))) return rc;
    cur = MRF;
  }
  if (sl.overflow) return fail(HFG_EIO, "internal: f16x3 scale slots exhausted");
  // lrelu -> conv_post -> tanh  (models/hifigan.py:254-256)
  {
    const Layer& Lp = h->layers[h->conv_post];
    const int64_t L = sh.L.back();
    const char* name = nullptr;
    ln.begin(2.0 * Lp.C_in * 7 * (double)L * B, 4.0 * B * L * (Lp.C_in + 1));
    hipError_t e = hfg::launch_conv_post(cur, (int64_t)Lp.C_in * L, Lp.C_in, (int)L,
                                         h->packed_dev + Lp.w_off, h->packed_dev + Lp.b_off, wav,
                                         lens_at(c.n_up), post_slope_of(h), (int)B, stream, &name);
    ln.end(name);
    if (e != hipSuccess) return fail(HFG_EIO, "launch conv_post: %s", hipGetErrorString(e));
  }
  return HFG_OK;
}

// The forward of a batch: utterances are independent, so a batch of B >= 2 runs as two
// halves on the caller's stream and an internal one (fork / join by events), each half
// with its own workspace slice.  Each wav is bitwise the same as in a one-stream run.
int forward_split(hfg_handle* h, const float* mel, int64_t B, int64_t T,
                  const hfg_forward_opts* o, float* wav, int64_t out_len, void* ws, size_t ws_len,
                  hipStream_t stream) {
  ++h->fwd_count;
  h->halves = split_batch(h, B, T) ? 2 : 1;
  if (h->halves == 1)
    return forward_impl(h, mel, B, T, o, wav, out_len, ws, ws_len, stream, 0, nullptr, true);
  if (B <= 0 || T <= 0) return fail(HFG_EINVAL, "B and T must be > 0");
  if (ws_len < ws_bytes_for(h, B, T)) return fail(HFG_EINVAL, "workspace too small");
  if (!h->aux) {
    hipError_t e = hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->join_ev, hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(e, "create split stream");
  }
  const int64_t B1 = (B + 1) / 2, B2 = B - B1;
  const size_t w1 = ws_part_bytes(h, B1, T);
  hipStream_t s0 = stream, s1 = h->aux;
  hipError_t e = hipEventRecord(h->fork_ev, stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(s1, h->fork_ev, 0);
  if (e != hipSuccess) return hip_fail(e, "fork");
  int rc = forward_impl(h, mel, B1, T, o, wav, out_len, ws, w1, s0, 0);
  if (rc) return rc;
  hfg_forward_opts o2{};
  if (o) {
    o2 = *o;
    if (o->lengths) o2.lengths = o->lengths + B1;
  }
  rc = forward_impl(h, mel + (size_t)B1 * h->cfg.n_mels * T, B2, T, o ? &o2 : nullptr,
                    wav + (size_t)B1 * out_len, out_len, static_cast<char*>(ws) + w1,
                    ws_len - w1, s1, 1);
  e = hipEventRecord(h->join_ev, s1);
  if (e == hipSuccess) e = hipStreamWaitEvent(stream, h->join_ev, 0);
  if (e != hipSuccess) return hip_fail(e, "join");
  return rc;
}

int create_impl(const hfg_config* cfg, bool mrf_only, int device, hfg_handle** out) {
  if (!out) return fail(HFG_EINVAL, "out is NULL");
  *out = nullptr;
  int rc = validate_config(cfg);
  if (rc) return rc;
  if (device >= 0) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(HFG_ENODEV, "no HIP device available");
    if (device >= n) return fail(HFG_ENODEV, "device %d out of range (%d devices)", device, n);
  }
  hfg_handle* h = new (std::nothrow) hfg_handle();
  if (!h) return fail(HFG_ENOMEM, "out of host memory");
  h->cfg = *cfg;
  h->mrf_only = mrf_only;
  h->device = device;
#if HFG_ABLATE
  sched_apply("DEBUG_FLAGS", &h->dbg_flags);
#endif
  sched_apply("RB_PERSIST", &h->rb_persist);
  if (device >= 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        n > 0)
      h->n_cu = n;
  }
  // knobs of earlier rounds' schedules that no longer exist: say so instead of silently
  // running the default schedule under a variant's label
  {
    static const char* const removed[] = {
        "HFG_SPLIT_MIN", "HFG_SPLIT_LAG", "HFG_SPLIT_STAGGER", "HFG_RB_NCH", "HFG_RB_NCH_BLOCKS",
        "HFG_UPS_SMALL_ROWS", "HFG_RB_WMR", "HFG_RB_WM", "HFG_RB_SPLIT_MIN", "HFG_RB_SPLIT_TH",
        "HFG_RB64_NARROW", "HFG_MFMA16", "HFG_EPI_LDS", "HFG_AREG", "HFG_UPS_SWIZZLE",
        "HFG_UPS_PLANES", "HFG_UPS_NT", "HFG_UPS_NT2", "HFG_THIN_MFMA", "HFG_POST4",
        "HFG_SMALL_GRID", "HFG_RB_WN32", "HFG_C16", "HFG_BF16X3_BIGTILE"};
    static std::once_flag warned;
    std::call_once(warned, [] {
      for (const char* k : removed)
        if (getenv(k))
          fprintf(stderr, "[hifigan_hip] %s is set but no longer read (a removed schedule knob); "
                          "the default schedule runs\n", k);
      // the round 1-5 environment knobs: now hfg_debug_schedule_set only
      char env[64];
      for (const SchedKnob& k : kSchedKnobs) {
        snprintf(env, sizeof(env), "HFG_%s", k.name);
        if (getenv(env))
          fprintf(stderr, "[hifigan_hip] %s is set but the library no longer reads its schedule "
                          "from the environment (hfg_debug_schedule_set); the default schedule "
                          "runs\n", env);
      }
    });
  }
  // schedule choices the parity suites compare (each bitwise invisible, or for the fused
  // ResBlocks a different rounding order): overridden only through hfg_debug_schedule_set
  sched_apply("FUSED_RB", &h->use_fused_rb);
  sched_apply("FUSE_POST", &h->fuse_post);
  sched_apply("RB_SPLIT", &h->rb_split);
  sched_apply("SMALL_TILE", &h->small_tile);
  sched_apply("RB_CONC", &h->rb_conc);
  sched_apply("UPS_FRAMES", &h->ups_frames);
  sched_apply("SPLIT", &h->split);
  sched_apply("AREG_TALL", &h->areg_tall);
  h->fmt = split_fmt(cfg->dtype);
  // bf16-valued weights: their lo plane is zero, the kernels skip lo(w) * hi(x)
  if (cfg->dtype == HFG_DTYPE_BF16W) h->np = 2;
  rc = build_layers(h);
  if (rc) {
    delete h;
    return rc;
  }
  *out = h;
  return HFG_OK;
}

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

#ifndef HFG_SRC_HASH
#define HFG_SRC_HASH "unknown"
#endif
// "... src:<16 hex>": sha256 of the build inputs (csrc/, include/, flags), computed by
// build.py and compiled in, so a loaded binary can be matched to its source tree
const char* hfg_version(void) {
  return "hifigan_hip 0.4.0 gfx950 f16x3-mfma fp32-mfma bf16x3-mfma src:" HFG_SRC_HASH;
}

const char* hfg_last_error(void) { return g_err.c_str(); }

int hfg_debug_schedule_set(const char* knob, int value) {
  const SchedKnob* k = sched_knob(knob);
  if (!k) return fail(HFG_EINVAL, "unknown schedule knob '%s'", knob ? knob : "(null)");
  if (value < k->lo || value > k->hi)
    return fail(HFG_EINVAL, "schedule knob %s = %d out of range [%d, %d]%s", k->name, value,
                k->lo, k->hi,
                !strcmp(k->name, "UPS_FRAMES") && value == 0
                    ? " (0, the polyphase-only upsampler schedule, was removed in round 4)"
                    : "");
  std::lock_guard<std::mutex> lk(g_sched_mu);
  g_sched[k->name] = value;
  return HFG_OK;
}

int hfg_debug_schedule_clear(const char* knob) {
  if (knob && !sched_knob(knob)) return fail(HFG_EINVAL, "unknown schedule knob '%s'", knob);
  std::lock_guard<std::mutex> lk(g_sched_mu);
  if (knob)
    g_sched.erase(knob);
  else
    g_sched.clear();
  return HFG_OK;
}

int hfg_debug_schedule_get(const char* knob, int* value) {
  if (!sched_knob(knob) || !value) return fail(HFG_EINVAL, "unknown schedule knob or NULL value");
  std::lock_guard<std::mutex> lk(g_sched_mu);
  auto it = g_sched.find(knob);
  if (it == g_sched.end()) return 0;
  *value = it->second;
  return 1;
}

int hfg_create(const hfg_config* cfg, int device, hfg_handle** out) {
  return create_impl(cfg, false, device, out);
}

int hfg_mrf_create(const hfg_mrf_config* mc, int device, hfg_handle** out) {
  if (!out) return fail(HFG_EINVAL, "out is NULL");
  *out = nullptr;
  if (!mc) return fail(HFG_EINVAL, "config is NULL");
  if (mc->channels <= 0) return fail(HFG_EINVAL, "channels must be > 0");
  // the generator-level config of one MRF stage: validate_config checks the ResBlock lists
  hfg_config c{};
  c.n_mels = 1;
  c.n_up = 1;
  c.up_rates[0] = 1;
  c.up_kernels[0] = 1;
  c.c0 = 2 * mc->channels;
  c.n_res = mc->n_res;
  for (int j = 0; j < HFG_MAX_RES; ++j) {
    c.res_kernels[j] = mc->res_kernels[j];
    c.n_dil[j] = mc->n_dil[j];
    for (int m = 0; m < HFG_MAX_DIL; ++m) c.dil[j][m] = mc->dil[j][m];
  }
  c.dtype = mc->dtype;
  c.resblock_type = mc->resblock_type;
  return create_impl(&c, true, device, out);
}

void hfg_destroy(hfg_handle* h) {
  if (!h) return;
  {
    DeviceGuard g(h->device);
    if (h->device >= 0) {
      recycle_prof(h);
      for (auto e : h->event_pool) (void)hipEventDestroy(e);
      if (h->packed_dev) (void)hipFree(h->packed_dev);
      if (h->ws) (void)hipFree(h->ws);
      if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
      if (h->join_ev) (void)hipEventDestroy(h->join_ev);
      if (h->aux) (void)hipStreamDestroy(h->aux);
      for (int part = 0; part < 2; ++part) {
        if (h->rb_fork[part]) (void)hipEventDestroy(h->rb_fork[part]);
        for (int j = 0; j < HFG_MAX_RES; ++j) {
          if (h->rb_join[part][j]) (void)hipEventDestroy(h->rb_join[part][j]);
          if (h->rb_aux[part][j]) (void)hipStreamDestroy(h->rb_aux[part][j]);
        }
      }
    }
  }
  delete h;
}

int hfg_num_params(const hfg_handle* h) { return h ? (int)h->param_order.size() : 0; }

int hfg_set_weight(hfg_handle* h, const char* name, const void* data, const int64_t* shape,
                   int ndim, int is_device) {
  if (!h || !name || !data || (!shape && ndim > 0))
    return fail(HFG_EINVAL, "NULL argument to hfg_set_weight");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  std::string key(name);
  std::vector<int64_t> shp(shape, shape + ndim);
  size_t n = 1;
  for (auto d : shp) {
    if (d < 0) return fail(HFG_EINVAL, "negative dimension for '%s'", name);
    n *= (size_t)d;
  }
  std::vector<float> buf(n);
  if (is_device) {
    if (h->device < 0) return fail(HFG_EINVAL, "device pointer given to a host-only handle");
    DeviceGuard g(h->device);
    hipError_t e = hipMemcpy(buf.data(), data, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(set_weight)");
  } else {
    std::memcpy(buf.data(), data, n * sizeof(float));
  }
  auto ends_with = [&](const char* suf) {
    size_t l = strlen(suf);
    return key.size() > l && key.compare(key.size() - l, l, suf) == 0;
  };
  // a ResBlock key of the other block type: say which layout this handle holds
  const bool pair_key = key.find(".convs1.") != std::string::npos ||
                        key.find(".convs2.") != std::string::npos;
  if (h->cfg.resblock_type == 1 && pair_key)
    return fail(HFG_EINVAL, "key '%s': this handle holds ResBlock2 blocks (resblock_type 1), whose "
                "parameters are resblocks.{j}.convs.{m}.*, not convs1 / convs2", name);
  if (h->cfg.resblock_type == 0 && key.find(".convs.") != std::string::npos)
    return fail(HFG_EINVAL, "key '%s': this handle holds the reference's ResBlock (resblock_type "
                "0), whose parameters are resblocks.{j}.convs1.{m}.* / convs2.{m}.*; create it "
                "with resblock_type 1 for ResBlock2's convs.{m}", name);
  if (ends_with(".weight_g") || ends_with(".weight_v")) {
    // apply_weight_norm layout (models/hifigan.py:274-283): w = g * v / ||v||, dim=0
    const std::string mod = key.substr(0, key.size() - 9);
    auto it = h->params.find(mod + ".weight");
    if (it == h->params.end()) return fail(HFG_EINVAL, "unknown key '%s'", name);
    const auto& wshape = it->second.shape;
    if (ends_with(".weight_v")) {
      if (shp != wshape) return fail(HFG_EINVAL, "shape mismatch for '%s'", name);
    } else {
      std::vector<int64_t> gshape(wshape.size(), 1);
      gshape[0] = wshape[0];
      if (shp != gshape) return fail(HFG_EINVAL, "shape mismatch for '%s'", name);
    }
    Param& part = h->wn_parts[key];
    part.shape = shp;
    part.data = std::move(buf);
    part.set = true;
    auto g = h->wn_parts.find(mod + ".weight_g");
    auto v = h->wn_parts.find(mod + ".weight_v");
    if (g != h->wn_parts.end() && v != h->wn_parts.end() && g->second.set && v->second.set) {
      Param& W = it->second;
      const size_t d0 = (size_t)wshape[0];
      const size_t inner = v->second.data.size() / d0;
      W.data.resize(v->second.data.size());
      for (size_t i = 0; i < d0; ++i) {
        double ss = 0.0;
        const float* vv = v->second.data.data() + i * inner;
        for (size_t q = 0; q < inner; ++q) ss += (double)vv[q] * vv[q];
        const double scale = (double)g->second.data[i] / std::sqrt(ss);
        for (size_t q = 0; q < inner; ++q) W.data[i * inner + q] = (float)(vv[q] * scale);
      }
      W.set = true;
      h->dirty = true;
    }
    return HFG_OK;
  }
  auto it = h->params.find(key);
  if (it == h->params.end()) return fail(HFG_EINVAL, "unknown key '%s'", name);
  if (shp != it->second.shape) {
    std::string want;
    for (auto d : it->second.shape) want += std::to_string(d) + ",";
    return fail(HFG_EINVAL, "shape mismatch for '%s' (expected [%s])", name, want.c_str());
  }
  it->second.data = std::move(buf);
  it->second.set = true;
  h->dirty = true;
  return HFG_OK;
}

int hfg_commit_weights(hfg_handle* h) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  return do_commit(h);
}

int64_t hfg_out_len(const hfg_handle* h, int64_t T) {
  if (!h || T <= 0 || h->mrf_only) return -1;
  return shapes_for(h, 1, T).L.back();
}

size_t hfg_workspace_bytes(const hfg_handle* h, int64_t B, int64_t T) {
  if (!h || B <= 0 || T <= 0 || h->mrf_only) return 0;
  return ws_bytes_for(h, B, T);
}

int hfg_reserve(hfg_handle* h, int64_t B, int64_t T) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle has no generator workspace");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle");
  if (B <= 0 || T <= 0) return fail(HFG_EINVAL, "B and T must be > 0");
  const size_t need = ws_bytes_for(h, B, T);
  if (need <= h->ws_bytes) return HFG_OK;
  DeviceGuard g(h->device);
  if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
  if (h->ws) {
    (void)hipDeviceSynchronize();
    (void)hipFree(h->ws);
  }
  h->ws = nullptr;
  h->ws_bytes = 0;
  hipError_t e = hipMalloc(&h->ws, need);
  if (e != hipSuccess) return fail(HFG_ENOMEM, "hipMalloc(workspace %zu B): %s", need,
                                   hipGetErrorString(e));
  h->ws_bytes = need;
  return HFG_OK;
}

int hfg_forward_ex(hfg_handle* h, const float* mel, int64_t B, int64_t T,
                   const hfg_forward_opts* opts, float* wav, int64_t out_len, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle: use hfg_mrf_forward");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (!workspace) return fail(HFG_EINVAL, "workspace is NULL");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
  if (h->dirty) {
    int rc = do_commit(h);
    if (rc) return rc;
  }
  return forward_split(h, mel, B, T, opts, wav, out_len, workspace, workspace_bytes,
                       reinterpret_cast<hipStream_t>(stream));
}

int hfg_forward_ws(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                   int64_t out_len, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle: use hfg_mrf_forward");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (!workspace) return fail(HFG_EINVAL, "workspace is NULL");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
  if (h->dirty) {
    int rc = do_commit(h);
    if (rc) return rc;
  }
  return forward_split(h, mel, B, T, nullptr, wav, out_len, workspace, workspace_bytes,
                       reinterpret_cast<hipStream_t>(stream));
}

int hfg_forward(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                int64_t out_len, void* stream) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle: use hfg_mrf_forward");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  int rc = hfg_reserve(h, B, T);
  if (rc) return rc;
  return hfg_forward_ws(h, mel, B, T, wav, out_len, h->ws, h->ws_bytes, stream);
}

// ---- one MRF / one ResBlock (MRF-only handles, hfg_mrf_create) ---------------
namespace {
int mrf_check(hfg_handle* h, const float* x, int64_t B, int64_t L, float* y, void* ws) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (!h->mrf_only) return fail(HFG_EINVAL, "not an MRF handle (hfg_mrf_create)");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (!x || !y || !ws) return fail(HFG_EINVAL, "x / y / workspace pointer is NULL");
  if (x == y) return fail(HFG_EINVAL, "y must not alias x");
  if (B <= 0 || L <= 0) return fail(HFG_EINVAL, "B and L must be > 0");
  if ((int64_t)h->stages[0].C * L >= ((int64_t)1 << 30))
    return fail(HFG_EINVAL, "per-item activation reaches 2^30 elements");
  return HFG_OK;
}
size_t mrf_ws_bytes(const hfg_handle* h, int64_t B, int64_t L) {
  const size_t one = ((sizeof(float) * (size_t)B * h->stages[0].C * (size_t)L) + 255) & ~(size_t)255;
  return 2 * one + slots_bytes(h, B);
}
int mrf_run(hfg_handle* h, int only_j, const float* x, int64_t B, int64_t L, float* y, void* ws,
            size_t ws_bytes, void* stream) {
  int rc = mrf_check(h, x, B, L, y, ws);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (ws_bytes < mrf_ws_bytes(h, B, L)) return fail(HFG_EINVAL, "workspace too small");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
  if (h->dirty && (rc = do_commit(h))) return rc;
  ++h->fwd_count;
  h->halves = 1;
  const size_t one = (mrf_ws_bytes(h, B, L) - slots_bytes(h, B)) / 2;
  float* R = static_cast<float*>(ws);
  float* Tb = R + one / sizeof(float);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Slots sl;
  Launcher ln{h, st, 0};
  ln.sl = &sl;
  uint32_t* ax = nullptr;
  if (h->fmt == hfg::kFmtF16) {
    // the caller's x: its per-item max |value| by an absmax pass
    sl.base = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + 2 * one);
    sl.n = n_slots(h);
    sl.B = B;
    hipError_t e = hipMemsetAsync(sl.base, 0, slots_bytes(h, B), st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(scale slots)");
    ax = ln.take();
    e = hfg::launch_absmax(x, (int64_t)h->stages[0].C * L, L, 1, h->stages[0].C, (int)L, nullptr,
                           (int)B, ax, st);
    if (e != hipSuccess) return fail(HFG_EIO, "launch absmax: %s", hipGetErrorString(e));
  }
  rc = run_mrf(h, ln, h->stages[0], x, B, L, R, Tb, y, nullptr, only_j, ax, nullptr);
  if (rc == HFG_OK && sl.overflow) return fail(HFG_EIO, "internal: f16x3 scale slots exhausted");
  return rc;
}
}  // namespace

size_t hfg_mrf_workspace_bytes(const hfg_handle* h, int64_t B, int64_t L) {
  if (!h || !h->mrf_only || B <= 0 || L <= 0) return 0;
  return mrf_ws_bytes(h, B, L);
}

int hfg_mrf_forward(hfg_handle* h, const float* x, int64_t B, int64_t L, float* y,
                    void* workspace, size_t workspace_bytes, void* stream) {
  return mrf_run(h, -1, x, B, L, y, workspace, workspace_bytes, stream);
}

int hfg_resblock_forward(hfg_handle* h, int j, const float* x, int64_t B, int64_t L, float* y,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (h && (j < 0 || j >= h->cfg.n_res)) return fail(HFG_EINVAL, "resblock index %d out of range", j);
  return mrf_run(h, j, x, B, L, y, workspace, workspace_bytes, stream);
}

// ---- content hash of parameter tensors -----------------------------------------
int hfg_checksum32(const void* const* ptrs, const int64_t* nbytes, int n, uint32_t* out,
                   void* stream) {
  if (n < 0 || (n > 0 && (!ptrs || !nbytes || !out))) return fail(HFG_EINVAL, "bad arguments");
  if (n == 0) return HFG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(out, 0, sizeof(uint32_t) * (size_t)n, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(checksum)");
  for (int base = 0; base < n; base += hfg::kChecksumMax) {
    hfg::ChecksumArgs a{};
    a.base = base;
    a.count = std::min(hfg::kChecksumMax, n - base);
    for (int i = 0; i < a.count; ++i) {
      if (nbytes[base + i] % 4 != 0 || (nbytes[base + i] > 0 && !ptrs[base + i]))
        return fail(HFG_EINVAL, "tensor %d: size must be a multiple of 4 bytes", base + i);
      a.p[i] = static_cast<const uint32_t*>(ptrs[base + i]);
      a.n[i] = nbytes[base + i] / 4;
    }
    e = hfg::launch_checksum(a, out, st);
    if (e != hipSuccess) return hip_fail(e, "launch checksum");
  }
  return HFG_OK;
}

int hfg_set_streams(hfg_handle* h, int n) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (n != 1 && n != 2) return fail(HFG_EINVAL, "streams must be 1 or 2 (got %d)", n);
  h->split = n;
  return HFG_OK;
}

int hfg_set_profiling(hfg_handle* h, int enable) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  h->profiling = enable != 0;
  return HFG_OK;
}

int hfg_profile_reset(hfg_handle* h) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  DeviceGuard g(h->device);
  for (auto& r : h->prof)
    if (r.e1) (void)hipEventSynchronize(r.e1);
  recycle_prof(h);
  return HFG_OK;
}

int hfg_profile_summary(hfg_handle* h, char* buf, size_t buflen) {
  if (!h || !buf || buflen == 0) return fail(HFG_EINVAL, "bad arguments");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  DeviceGuard g(h->device);
  struct Agg {
    int launches = 0;
    double ms = 0, flop = 0, bytes = 0;
  };
  std::map<std::string, Agg> agg;
  // a split forward's two half-batch dispatches of one layer count as one launch: its
  // FLOP / bytes summed over the halves, its time the union of the two intervals
  std::map<std::tuple<int, int>, std::pair<const ProfRec*, const ProfRec*>> pairs;
  for (auto& r : h->prof) {
    if (!r.e0 || !r.e1 || !r.label) continue;
    auto& pr = pairs[std::make_tuple(r.fwd, r.seq)];
    (r.part == 0 ? pr.first : pr.second) = &r;
  }
  auto elapsed = [](hipEvent_t a, hipEvent_t b, float* ms) -> hipError_t {
    hipError_t e = hipEventSynchronize(b);
    if (e == hipSuccess) e = hipEventSynchronize(a);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, a, b);
    return e;
  };
  for (auto& kv : pairs) {
    const ProfRec* A = kv.second.first ? kv.second.first : kv.second.second;
    const ProfRec* Bq = kv.second.first ? kv.second.second : nullptr;
    float dA = 0.f;
    hipError_t e = elapsed(A->e0, A->e1, &dA);
    if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
    double ms = dA, flop = A->flop, bytes = A->bytes;
    if (Bq) {
      // B's start / end relative to A's start (either order)
      float s0 = 0.f, s1 = 0.f;
      if (elapsed(A->e0, Bq->e0, &s0) != hipSuccess || s0 < 0.f) {
        float r = 0.f;
        if (elapsed(Bq->e0, A->e0, &r) != hipSuccess) return fail(HFG_EIO, "event order");
        s0 = -r;
      }
      float dB = 0.f;
      e = elapsed(Bq->e0, Bq->e1, &dB);
      if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
      s1 = s0 + dB;
      ms = std::max<double>(dA, s1) - std::min<double>(0.0, s0);
      flop += Bq->flop;
      bytes += Bq->bytes;
    }
    Agg& a = agg[A->label];
    a.launches++;
    a.ms += ms;
    a.flop += flop;
    a.bytes += bytes;
  }
  std::string s = "{";
  bool first = true;
  for (auto& kv : agg) {
    char line[512];
    snprintf(line, sizeof(line), "%s\"%s\": {\"launches\": %d, \"ms\": %.6f, \"flop\": %.6e, "
             "\"bytes\": %.6e}", first ? "" : ", ", kv.first.c_str(), kv.second.launches,
             kv.second.ms, kv.second.flop, kv.second.bytes);
    s += line;
    first = false;
  }
  s += "}";
  if (s.size() + 1 > buflen) return fail(HFG_EINVAL, "buffer too small (%zu needed)", s.size() + 1);
  memcpy(buf, s.c_str(), s.size() + 1);
  return HFG_OK;
}

// ---- inspection helpers (not part of the public header's compute API) ------
// Copy the packed host image of layer `name` (module prefix) for host tests.
int hfg_debug_packed_layer(hfg_handle* h, const char* mod, float* out, size_t cap,
                           int64_t* info) {
  if (!h || !mod) return fail(HFG_EINVAL, "NULL argument");
  for (auto& L : h->layers) {
    if (L.mod != mod) continue;
    if (info) {
      info[0] = L.kind;
      info[1] = L.M;
      info[2] = L.KT;
      info[3] = L.tile;
      info[4] = L.m_tiles;
      info[5] = L.n_chunks;
      info[6] = (int64_t)L.w_len;
      info[7] = (int64_t)L.b_len;
      info[8] = L.CK;
      info[9] = L.kind == L_POST ? 0
                : L.prec == 1    ? hfg::kBf16x3Tiles[L.tile].MT()
                                 : kTiles[L.tile].MT();
    }
    if (!out) return HFG_OK;
    if (h->dirty) {
      int rc = do_commit(h);
      if (rc) return rc;
    }
    if (cap < L.w_len + L.b_len) return fail(HFG_EINVAL, "output buffer too small");
    memcpy(out, h->packed_host.data() + L.w_off, sizeof(float) * L.w_len);
    memcpy(out + L.w_len, h->packed_host.data() + L.b_off, sizeof(float) * L.b_len);
    return HFG_OK;
  }
  return fail(HFG_EINVAL, "unknown layer '%s'", mod);
}

// The f16x3 packing exponent of layer `mod` (0 in the other modes): set by the commit, so a
// handle with uncommitted weights commits first and returns its error (e.g. weights missing).
int hfg_debug_layer_exponent(hfg_handle* h, const char* mod, int* ew) {
  if (!h || !mod || !ew) return fail(HFG_EINVAL, "NULL argument");
  for (auto& L : h->layers) {
    if (L.mod != mod) continue;
    if (h->dirty) {
      int rc = do_commit(h);
      if (rc) return rc;
    }
    *ew = L.ew;
    return HFG_OK;
  }
  return fail(HFG_EINVAL, "unknown layer '%s'", mod);
}

int hfg_debug_packed_resblock(hfg_handle* h, int stage, int j, float* out, size_t cap,
                              int64_t* info) {
  if (!h || !info) return fail(HFG_EINVAL, "NULL argument");
  if (stage < 0 || stage >= (int)h->stages.size()) return fail(HFG_EINVAL, "stage out of range");
  const Stage& st = h->stages[stage];
  for (int i = 0; i < 8; ++i) info[i] = 0;
  if (j < 0 || j >= (int)st.rbs.size()) return fail(HFG_EINVAL, "resblock out of range");
  const RbFused& rb = st.rbs[j];
  if (!rb.fused) return HFG_OK;
  info[0] = 1;  // fused (resblock_bf16x3 stream order)
  info[1] = h->layers[rb.convs[0]].C_out;
  info[2] = rb.kt;
  info[3] = (int64_t)rb.convs.size();
  info[4] = rb.halo;
  info[5] = rb.W;
  info[6] = (int64_t)rb.w_len;
  info[7] = (int64_t)rb.b_len;
  if (!out) return HFG_OK;
  if (h->dirty) {
    int rc = do_commit(h);
    if (rc) return rc;
  }
  if (cap < rb.w_len + rb.b_len) return fail(HFG_EINVAL, "output buffer too small");
  memcpy(out, h->packed_host.data() + rb.w_off, sizeof(float) * rb.w_len);
  memcpy(out + rb.w_len, h->packed_host.data() + rb.b_off, sizeof(float) * rb.b_len);
  return HFG_OK;
}

int hfg_forward_taps(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                     int64_t out_len, void* workspace, size_t workspace_bytes,
                     float* const* taps, int n_taps, void* stream) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->device < 0 || h->mrf_only) return fail(HFG_EINVAL, "not a generator device handle");
  if (!workspace) return fail(HFG_EINVAL, "workspace is NULL");
  if (taps && n_taps != 1 + 2 * h->cfg.n_up)
    return fail(HFG_EINVAL, "n_taps must be 1 + 2 * n_up = %d", 1 + 2 * h->cfg.n_up);
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
  if (h->dirty) {
    int rc = do_commit(h);
    if (rc) return rc;
  }
  ++h->fwd_count;
  h->halves = 1;
  return forward_impl(h, mel, B, T, nullptr, wav, out_len, workspace, workspace_bytes,
                      reinterpret_cast<hipStream_t>(stream), 0, taps, !split_batch(h, B, T));
}

}  // extern "C"
