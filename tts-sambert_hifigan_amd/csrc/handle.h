// handle.h — what the host orchestration units share: the handle and its plan (layers,
// whole-ResBlock and thin-stage launches, packed-buffer offsets), the error channel, the
// schedule-knob table and the device guard (device_guard.h).
//   plan.cpp     config validation, the plan, shapes and workspace sizing (no HIP runtime call)
//   pack.cpp     weights -> the kernels' packed operand orders (host)
//   forward.cpp  the launch schedule, the weight upload
//   hifigan_capi.cpp  the C ABI of include/hifigan_hip.h, the parameter store
//   inspect_capi.cpp  the C ABI of include/hifigan_hip_inspect.h, the schedule-knob store
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hifigan_hip.h"
#include "../../include/hifigan_hip_inspect.h"
#include "device_guard.h"
#include "kernels.h"

namespace hfg_host {

// the calling thread's hfg_last_error text; returns code
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char* what);
// How a text-returning entry ends: s and its NUL into buf, or HFG_EINVAL naming the size needed
int return_text(const std::string& s, char* buf, size_t buflen);

// The largest batch of a forward: the batch is gridDim.z of the layer convs and gridDim.y of
// the whole-block, thin, post, combine and absmax kernels, both limited to 65535.  Every entry
// that takes B refuses a larger one before it launches or sizes anything.
constexpr int64_t kMaxBatch = 65535;

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
    {"RESAMPLE_TABLE", 0, 1},  // hfg_resample_ragged's filter table: 0 phase-major, 1 tap-major
};
// the override of `knob` into *v if one is set (else *v is left alone)
void sched_apply(const char* knob, int* v);
void sched_apply(const char* knob, bool* v);

enum LayerKind { L_CONV, L_UPS, L_POST };

// A region of the packed buffer, in floats; its length is its layout's size (pack_layout.h).
// len == 0: absent
struct PackRegion { size_t off = 0, len = 0; };

// One packing of a layer's weights and per-row biases for one tile of its kernel.
struct Packing {
  int tile, m_tiles, n_chunks;
  PackRegion w, b;
};

struct Layer {
  LayerKind kind;
  std::string mod;   // state_dict module prefix
  int C_in, C_out, k, dil, pad;
  int s, p;          // ConvTranspose1d stride / padding
  int M, KT, CK;     // GEMM view
  int prec;          // 0: fp32 MFMA kernel, 1: split-precision kernel (bf16x3 / f16x3)
  int ew = 0;        // f16x3: power-of-two exponent of this layer's weight packing
  // [0]: the layer's own tile; [1]: split-precision layers' second packing for the small-grid
  // tile (kBf16x3SmallTile), tile -1: none
  Packing pk[2] = {{0, 0, 0, {}, {}}, {-1, 0, 0, {}, {}}};
  // bf16x3 upsamplers with k = 2u: the output-frame kernel (ups_bf16x3.hip) on its own
  // packing, -1: none
  int ups_cfg = -1, m_tiles_f = 0;
  PackRegion wf, bf;
};

// f16x3, bf16x3 and bf16w run the split-operand MFMA kernels (f16x3 and bf16w in the f16
// format with power-of-two scales, bf16x3 in the bf16 format: bf16x3_common.h)
inline bool split_dtype(int dtype) {
  return dtype == HFG_DTYPE_F16X3 || dtype == HFG_DTYPE_BF16X3 || dtype == HFG_DTYPE_BF16W;
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

// One ResBlock run by resblock_bf16x3 (whole block per launch): its packed A stream (rb_nest,
// pack_layout.h) and biases [conv][C] in the packed buffer.
struct RbFused {
  std::vector<int> convs;     // layer indices in execution order conv1_0, conv2_0, conv1_1, ...
  bool fused = false;         // this ResBlock runs as one resblock_bf16x3 launch
  int kt = 0, halo = 0, W = 0, nwin = 0, wm = 1;  // window columns, row tiles per wave
  // split into two launches (convs [0, split) then [split, n)): each part's window pays
  // only its own receptive-field halo; the first writes x to scratch (0: one launch)
  int split = 0;
  int halo_p[2] = {0, 0}, W_p[2] = {0, 0};
  // the network's last MRF write may carry conv_post + tanh (forward.cpp, post_fusable): its
  // last launch is then exact on conv_post's radius more on either side
  bool post = false;
  int halo_post = 0, W_post = 0;
  PackRegion w, b;
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
  std::vector<PackRegion> thin_w;  // per conv (thin_nest, pack_layout.h)
  PackRegion thin_b;               // [conv][C]
  // bf16x3: the MFMA kernel's A stream, the convs of thin_mfma_nest one after another
  bool thin_mfma = false;
  PackRegion thin_m;
  std::vector<int> thin_m_conv;    // byte offset of each conv inside the stream
};

}  // namespace hfg_host

struct hfg_handle {
  hfg_config cfg;
  int device;  // -1: host-only handle (validation / packing inspection)
  // MRF-only handle (hfg_mrf_create): one stage of ResBlocks keyed "resblocks.{j}.*"
  // (the MRF module's own state_dict), no conv_pre / ups / conv_post
  bool mrf_only = false;
  // one forward at a time per handle: the split stream, its fork/join events and the
  // profiling records are shared state (ctypes releases the GIL around the call)
  std::recursive_mutex mu;
  std::vector<hfg_host::Layer> layers;
  int conv_pre = -1, conv_post = -1;
  std::vector<hfg_host::Stage> stages;
  std::map<std::string, hfg_host::Param> params;    // "<mod>.weight" / "<mod>.bias"
  std::map<std::string, hfg_host::Param> wn_parts;  // "<mod>.weight_g" / "<mod>.weight_v"
  std::vector<std::string> param_order;
  bool dirty = true;
  std::vector<float> packed_host;
  float* packed_dev = nullptr;
  size_t packed_dev_len = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  bool profiling = false;
  bool use_fused_rb = true;  // whole-ResBlock kernel for C in {32, 64, 128} (FUSED_RB=0:
                             // layer by layer; the parity suites compare both schedules)
  bool rb_split = true;      // whole-ResBlock split in two launches where it cuts >= 10 % of the
                             // halo recompute (k = 11 in V1; RB_SPLIT=0: one launch)
  bool fuse_post = true;     // conv_post + tanh inside the last C = 32 ResBlock launch
                             // (FUSE_POST=0: its own kernel; bitwise the same wav)
  int ups_frames = 1;        // k = 2u upsamplers on the output-frame kernel: 1 when its grid
                             // fills the chip, 2 always (UPS_FRAMES; the polyphase
                             // conv1d_bf16x3 path gives the bitwise same result)
  int fmt = 0;               // split format of the split kernels (bf16x3_common.h)
  int np = 3;                // MFMA products per multiply-add: 3, or 2 (bf16w: lo(w) = 0)
  int small_tile = -1;       // small-grid tile: -1 auto (grid < kSmallGridBlocks), 0 never,
                             // 1 always (SMALL_TILE; bitwise invisible)
  int dbg_flags = 0;  // DEBUG_FLAGS (kernel ablations, -DHFG_ABLATE=1 builds only)
  // RB_PERSIST (default 2): persistent grids for the one-block-per-CU ResBlock launches
  int rb_persist = 2;
  // AREG_TALL: layers whose rows are a multiple of 256 on the 256x128 AREG tile (6): each input
  // window staged once per 128 output columns instead of once per m-tile (bitwise tile 5)
  int areg_tall = 1;
  int n_cu = 256;      // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  int halves = 1;      // batch halves of the running forward (2: two streams share the CUs)
  // batch split over two HIP streams (SPLIT=1 disables): the two halves' launches
  // overlap, so one half's ramp-down / epilogue tail runs beside the other's main loops
  int split = 2;
  static constexpr int64_t kSplitMinFrames = 4096;  // batch frames from which a forward runs as
                                                    // two halves on two streams
  // concurrent ResBlocks for a stage whose grids leave CUs idle: fewer tile-3 blocks (128 rows
  // x 256 columns) per conv than this.  512 (the chip's tile-3 slots) until round 6; with the
  // cheaper mrf_combine, 2048 also takes the whole-ResBlock stages of mid-size single-stream
  // forwards (same-box sweep, profiles/r06/c1/c1_ab_cb.txt: 4 x 512 frames -3.7 %, 32 x 62
  // -1.6 %, 1 x 4096 -0.8 %, 1 x 8192 and 16 x 256 unchanged; 4096 cost 1 x 8192 +1.2 %)
  static constexpr int64_t kConcBlocks = 2048;
  hipStream_t aux = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  // concurrent ResBlocks of small forwards (RB_CONC: -1 auto, 0 off, 1 whenever the
  // workspace allows): per batch part, aux streams for ResBlocks 1.. and their events
  int rb_conc = -1;
  hipStream_t rb_aux[2][HFG_MAX_RES] = {};
  hipEvent_t rb_fork[2] = {};
  hipEvent_t rb_join[2][HFG_MAX_RES] = {};
  int fwd_count = 0;
  std::vector<hfg_host::ProfRec> prof;
  std::vector<hipEvent_t> event_pool;
};

namespace hfg_host {

// ---- plan.cpp ---------------------------------------------------------------
int validate_config(const hfg_config* c);
// Apply the schedule knobs to a handle whose cfg / mrf_only / device are set and build its
// plan: layers, stages, packed-buffer offsets.  HFG_EINVAL when a layer's taps x dilation
// is beyond every kernel's staging limits.
int plan_handle(hfg_handle* h);

struct Shapes {
  std::vector<int64_t> L;  // L[0] = T, L[i+1] = length after stage i
  int64_t item_elems;      // largest per-item activation (max over stages of C * L)
};
Shapes shapes_for(const hfg_handle* h, int64_t T);
bool stage_conc(const hfg_handle* h, const Stage& st, int64_t B, int64_t L);
bool split_batch(const hfg_handle* h, int64_t B, int64_t T);

// The workspace of a forward, stated once: plan.cpp computes it, the public sizes
// (hfg_workspace_bytes, hfg_mrf_workspace_bytes, hfg_reserve) are its totals, forward.cpp
// takes every pointer from it and hfg_debug_workspace prints it.  Offsets are bytes from the
// workspace's start, every region 256-byte aligned; bytes == 0: the region is absent.
struct WsRegion { size_t off = 0, bytes = 0; };
// R / Tb of a layer-per-launch ResBlock (Tb: also a split whole-ResBlock launch's x), and
// with concurrent ResBlocks the block's own output
struct WsRbRegions { WsRegion R, Tb, out; };
// One forward part: batch items [b0, b0 + B) on one stream.
struct WsPart {
  int64_t b0 = 0, B = 0;
  size_t off = 0, bytes = 0;
  WsRegion X;               // upsampled stage input
  WsRbRegions rb;           // R: running ResBlock state (also conv_pre output); rb.out: the
                            // MRF accumulator (absent in an MRF-only forward, which writes y)
  bool conc = false;        // some stage runs concurrent ResBlocks: rb_conc[0, n_res) present
  WsRbRegions rb_conc[HFG_MAX_RES];
  WsRegion table;           // per-stage valid lengths of a ragged batch, [n_up + 1][B] int32
  WsRegion slots;           // f16x3 scale slots, [n_slots][B][kAmaxSlotWords] uint32
};
struct WsLayout {
  int n_parts = 1;          // 2: the batch halves of a split forward, each on its stream
  WsPart part[2];
  size_t total = 0;
};
// A generator forward.  taps: hfg_forward_taps' one-stream forward, the whole batch as one
// part (with concurrent ResBlocks only where the split forward is one part too).
WsLayout ws_layout(const hfg_handle* h, int64_t B, int64_t T, bool taps);
// What hfg_workspace_bytes promises: room for either layout above.
size_t ws_bytes_for(const hfg_handle* h, int64_t B, int64_t T);
// An MRF-only forward: one part of rb.R, rb.Tb and the slots.
WsLayout mrf_ws_layout(const hfg_handle* h, int64_t B, int64_t L);
// f16x3 scale slots of one forward part: one [B] row of per-item max |value| per launch that
// commits a scale, handed out in launch order (forward.cpp, Launcher::act).  Those launches:
// the absmax pass over the caller's mel (or an MRF-only forward's x), conv_pre, every
// upsampler, every MRF output, and in a layer-by-layer ResBlock every conv but its last
// (whose output is the MRF write).  Fewer than layers + 2 n_up + 4 in every schedule; a
// schedule that asks for more fails with "scale slots exhausted".
int n_slots(const hfg_handle* h);

// ---- pack.cpp ---------------------------------------------------------------
// Every weight set -> h->packed_host (HFG_EAGAIN while one is missing); sets Layer::ew.
int pack_weights(hfg_handle* h);

// ---- hifigan_capi.cpp ---------------------------------------------------------
// what every generator forward entry refuses: NULL, host-only and MRF-only handles
int check_generator(const hfg_handle* h);

// ---- forward.cpp ------------------------------------------------------------
// pack_weights, then (device handles) the upload; clears h->dirty
int do_commit(hfg_handle* h);
void recycle_prof(hfg_handle* h);
// What every forward entry holds while it runs: the handle's lock and its device.
struct ForwardScope {
  std::lock_guard<std::recursive_mutex> lk;
  DeviceGuard g;
  explicit ForwardScope(hfg_handle* h) : lk(h->mu), g(h->device) {}
  // after the entry's own argument checks: the device is current, pending weights committed
  int ready(hfg_handle* h) {
    if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
    return h->dirty ? do_commit(h) : HFG_OK;
  }
};
// What the caller of a generator forward passed: mel [B][n_mels][T] (or BTC, opts) -> wav
// [B][out_len]; taps: hfg_forward_taps' stage-output copies (may be NULL there too).
struct FwdIo {
  const float* mel;
  int64_t B, T;
  const hfg_forward_opts* opts;
  float* wav;
  int64_t out_len;
  float* const* taps;
};
// Checks the arguments, lays the caller's workspace out (ws_layout) and refuses one smaller
// than that layout's total.  The batch halves run on two streams where split_batch says so;
// taps: hfg_forward_taps' forward, one stream.
int forward_run(hfg_handle* h, const FwdIo& io, void* ws, size_t ws_len, hipStream_t stream,
                bool taps);
// An MRF-only forward: x [part.B][C][L] -> y, the whole MRF (only_j < 0) or ResBlock only_j;
// ws: at least the total of the mrf_ws_layout that `part` is the one part of.
int mrf_run(hfg_handle* h, int only_j, const float* x, int64_t L, float* y, const WsPart& part,
            void* ws, hipStream_t stream);

}  // namespace hfg_host
