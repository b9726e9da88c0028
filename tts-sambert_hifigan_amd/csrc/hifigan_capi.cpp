// hifigan_capi.cpp — the C ABI of libhifigan_hip.so's compute boundary (include/hifigan_hip.h):
// argument checks, the handle's lock and device, the parameter store keyed by the reference
// state_dict names with weight-norm folding, and the error channel.  The plan, the packers and
// the launch schedule are plan.cpp, pack.cpp and forward.cpp (handle.h); the inspection entries
// and the schedule-knob store are inspect_capi.cpp.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <tuple>

#include "handle.h"
#include "json_writer.h"

using namespace hfg_host;

namespace {
thread_local std::string g_err;
}  // namespace

namespace hfg_host {
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
int return_text(const std::string& s, char* buf, size_t buflen) {
  if (s.size() + 1 > buflen) return fail(HFG_EINVAL, "buffer too small (%zu needed)", s.size() + 1);
  memcpy(buf, s.c_str(), s.size() + 1);
  return HFG_OK;
}
int check_generator(const hfg_handle* h) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle: use hfg_mrf_forward");
  return HFG_OK;
}
}  // namespace hfg_host

namespace {
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
  if (device >= 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        n > 0)
      h->n_cu = n;
  }
  rc = plan_handle(h);
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
  return shapes_for(h, T).L.back();
}

size_t hfg_workspace_bytes(const hfg_handle* h, int64_t B, int64_t T) {
  if (!h || B <= 0 || B > kMaxBatch || T <= 0 || h->mrf_only) return 0;
  return ws_bytes_for(h, B, T);
}

int hfg_reserve(hfg_handle* h, int64_t B, int64_t T) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle has no generator workspace");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle");
  if (B <= 0 || T <= 0) return fail(HFG_EINVAL, "B and T must be > 0");
  if (B > kMaxBatch) return fail(HFG_EINVAL, "B must be in [1, 65535] (got %lld)", (long long)B);
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
  int rc = check_generator(h);
  if (rc) return rc;
  ForwardScope scope(h);
  if (!workspace) return fail(HFG_EINVAL, "workspace is NULL");
  if ((rc = scope.ready(h))) return rc;
  return forward_run(h, FwdIo{mel, B, T, opts, wav, out_len, nullptr}, workspace, workspace_bytes,
                     reinterpret_cast<hipStream_t>(stream), false);
}

int hfg_forward_ws(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                   int64_t out_len, void* workspace, size_t workspace_bytes, void* stream) {
  return hfg_forward_ex(h, mel, B, T, nullptr, wav, out_len, workspace, workspace_bytes, stream);
}

int hfg_forward(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                int64_t out_len, void* stream) {
  int rc = check_generator(h);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if ((rc = hfg_reserve(h, B, T))) return rc;
  return hfg_forward_ws(h, mel, B, T, wav, out_len, h->ws, h->ws_bytes, stream);
}

// ---- one MRF / one ResBlock (MRF-only handles, hfg_mrf_create) ---------------
namespace {
int mrf_entry(hfg_handle* h, int only_j, const float* x, int64_t B, int64_t L, float* y, void* ws,
              size_t ws_bytes, void* stream) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (!h->mrf_only) return fail(HFG_EINVAL, "not an MRF handle (hfg_mrf_create)");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (!x || !y || !ws) return fail(HFG_EINVAL, "x / y / workspace pointer is NULL");
  if (x == y) return fail(HFG_EINVAL, "y must not alias x");
  if (B <= 0 || L <= 0) return fail(HFG_EINVAL, "B and L must be > 0");
  if (B > kMaxBatch) return fail(HFG_EINVAL, "B must be in [1, 65535] (got %lld)", (long long)B);
  if ((int64_t)h->stages[0].C * L >= ((int64_t)1 << 30))
    return fail(HFG_EINVAL, "per-item activation reaches 2^30 elements");
  ForwardScope scope(h);
  const WsLayout lay = mrf_ws_layout(h, B, L);
  if (ws_bytes < lay.total) return fail(HFG_EINVAL, "workspace too small");
  int rc = scope.ready(h);
  if (rc) return rc;
  return mrf_run(h, only_j, x, L, y, lay.part[0], ws, reinterpret_cast<hipStream_t>(stream));
}
}  // namespace

size_t hfg_mrf_workspace_bytes(const hfg_handle* h, int64_t B, int64_t L) {
  if (!h || !h->mrf_only || B <= 0 || B > kMaxBatch || L <= 0) return 0;
  return mrf_ws_layout(h, B, L).total;
}

int hfg_mrf_forward(hfg_handle* h, const float* x, int64_t B, int64_t L, float* y,
                    void* workspace, size_t workspace_bytes, void* stream) {
  return mrf_entry(h, -1, x, B, L, y, workspace, workspace_bytes, stream);
}

int hfg_resblock_forward(hfg_handle* h, int j, const float* x, int64_t B, int64_t L, float* y,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (h && (j < 0 || j >= h->cfg.n_res)) return fail(HFG_EINVAL, "resblock index %d out of range", j);
  return mrf_entry(h, j, x, B, L, y, workspace, workspace_bytes, stream);
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
  JsonWriter js;
  js.begin_object();
  for (auto& kv : agg) {
    js.key(kv.first).begin_object().integer("launches", kv.second.launches);
    js.key("ms").real("%.6f", kv.second.ms).key("flop").real("%.6e", kv.second.flop);
    js.key("bytes").real("%.6e", kv.second.bytes).end_object();
  }
  js.end_object();
  return return_text(js.str(), buf, buflen);
}

}  // extern "C"
