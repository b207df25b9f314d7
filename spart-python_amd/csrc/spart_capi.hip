// libspart_hip.so: the C ABI declared in include/spart_hip.h (host side: context, table
// derivation, workspace carving, kernel launches).  No torch types, no allocation on the
// call path (graph-capturable), caller owns every buffer.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/spart_hip.h"
#include "spart_bands_f32.h"
#include "spart_kernels.h"
#include "spart_lut.h"
#include "spart_refine.h"
#include "spart_refine_posterior.h"
#include "spart_refine_views.h"
#include "spart_refine_mix.h"
#include "spart_refine_tiles.h"
#include "spart_refine_series.h"
#include "spart_sobol.h"
#include "spart_vjp.h"
#include "spart_sample.h"
#include "spart_products.h"
#include "spart_refine_leaf.h"

using namespace spart;

struct SideLane {
  hipStream_t caller = nullptr, side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
struct WsUse {
  const char* base = nullptr;
  size_t bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  bool captured = false;             // `done` was recorded into a stream capture: it orders nothing outside that graph
};
constexpr size_t MAX_LANES = 32;     // caller streams with their own side stream (further streams run the columns in line;
                                     // stated in include/spart_hip.h)
constexpr size_t WS_PRUNE_AT = 16;   // (workspace, stream) records kept before completed ones are looked for and recycled

struct spart_ctx {
  int device = 0;
  float* tabF = nullptr;    // (NTAB, NWL)
  double* tabD = nullptr;   // (NTAB, NWL)
  double* Ea = nullptr;     // (NWL)
  double ea_par = 0.0, ea_all = 0.0;   // sum of Ea over bands 0 ... 300 / 0 ... 2000, float64, ascending (spart_products)
  int nb = 0;
  int pf = NWLS, po = NWL;  // row pitch (elements) of the 2162- / 2001-wide spectrum arrays (spart_ctx_set_row_pitch)
  int* band0 = nullptr;      // (nb) evaluation index of the np.interp support point at / below the band centre (k_columns)
  int* band1 = nullptr;      // (nb) ... of the next one (== band0 when the centre is a grid point)
  double* frac = nullptr;    // (nb)
  double* coef = nullptr;    // (48, nb)
  double* econv = nullptr;   // (nb)
  // compressed SRF support of every band (spart_srf_support) and the deal of the bands to k_columns_srf's waves
  int* srf_start = nullptr;  // (nb + 1)
  int* srf_ev = nullptr;     // (srf_start[nb]) evaluation indices, ascending within a band
  double* srf_q = nullptr;   // (srf_start[nb]) summed weight of each
  double* srf_Q = nullptr;   // (nb) sum of the band's weights
  int* srf_deal = nullptr;   // (nb rounded up to a multiple of COL_WAVES): srf_deal()
  std::vector<double> econv_host;
  // Everything below is mutable per-call state, guarded by `mu`: an entry point holds it while it checks the workspace
  // and issues its launches (microseconds; the GPU work itself stays asynchronous), so calls on ONE context may come from
  // any number of host threads and streams.
  std::mutex mu;
  // The column kernel (k_columns) runs on a side stream beside the full-band kernel (fork / join
  // with two events; spart_run_batch stays asynchronous on the caller's stream).  One lane PER CALLER STREAM, created on
  // first use: two caller streams never share a side stream or an event pair, and a stream under HIP-graph capture
  // pulls only its own side stream into the capture.
  bool side_enabled = true;
  std::vector<SideLane> lanes;
  // Last use of every workspace recently handed in: (range, stream, completion event).  A call that gets a workspace
  // still owned by a call on ANOTHER stream is ordered after it (hipStreamWaitEvent), so sharing one workspace between
  // streams is slow but never a race; if the order cannot be expressed the call fails with SPART_ERR_INVALID.
  std::vector<WsUse> ws_uses;
  // optional timing of the dominant kernel (k_bands): event pairs recorded on the caller's stream
  bool profile = false;
  std::vector<hipEvent_t> ev;   // NEV events per timed call (run_impl)
  size_t ev_used = 0;
  std::vector<char> ev_forked;  // per timed call: the column kernel ran on the side stream
};

constexpr size_t NEV = 4;        // events per timed spart_run_batch call: 3 stage intervals

// the text of the last error raised ON THE CALLING THREAD (spart_last_error): per thread, so that concurrent calls on one
// context cannot garble each other's message
static thread_local char g_err[512] = {0};

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, 512, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return fail(SPART_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_));           \
  } while (0)

namespace {

// Optional ROCTX ranges around the stages of spart_run_batch (the counterpart of the reference's NVTX
// annotations, SPART.py:191-227).  Never a hard dependency: the marker library is looked up with dlopen
// only when SPART_ROCTX=1 is set, and its absence is silent.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* e = std::getenv("SPART_ROCTX");
    if (!e || e[0] != '1') return;
    for (const char* name : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (!h) continue;
      push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
      pop = (int (*)())dlsym(h, "roctxRangePop");
      if (push && pop) return;
      push = nullptr;
      pop = nullptr;
    }
  }
};
Roctx& roctx() {
  static Roctx r;
  return r;
}
struct Range {
  bool on;
  explicit Range(const char* name) : on(roctx().push != nullptr) {
    if (on) roctx().push(name);
  }
  ~Range() {
    if (on) roctx().pop();
  }
};

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) ok = false;
    if (ok && prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// ---- per-call state of a context (all under ctx->mu)
// the side stream + event pair of caller stream `st`, created on first use; nullptr = run the columns in line
SideLane* lane_for(spart_ctx* ctx, hipStream_t st) {
  if (!ctx->side_enabled) return nullptr;
  for (SideLane& l : ctx->lanes)
    if (l.caller == st) return &l;
  if (ctx->lanes.size() >= MAX_LANES) return nullptr;
  SideLane l;
  l.caller = st;
  if (hipStreamCreateWithFlags(&l.side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&l.fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&l.join, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    if (l.fork) (void)hipEventDestroy(l.fork);
    if (l.join) (void)hipEventDestroy(l.join);
    if (l.side) (void)hipStreamDestroy(l.side);
    return nullptr;
  }
  ctx->lanes.push_back(l);
  return &ctx->lanes.back();
}

// Before a call's first launch: order it after every call that used an overlapping workspace range on ANOTHER stream.
int ws_acquire(spart_ctx* ctx, const char* base, size_t bytes, hipStream_t st, const char* who) {
  for (const WsUse& u : ctx->ws_uses) {
    if (u.stream == st || base >= u.base + u.bytes || u.base >= base + bytes) continue;
    const hipError_t e = hipStreamWaitEvent(st, u.done, 0);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(SPART_ERR_INVALID, "%s: the workspace is in use by a call on another stream and this call cannot be "
                  "ordered after it (%s): give every stream its own workspace", who, hipGetErrorString(e));
    }
  }
  return SPART_OK;
}
// After a call's last launch: remember (range, stream) and record its completion event.  A record is only ever recycled
// when the use it stands for HAS COMPLETED (hipEventQuery) or can order nothing (its event went into a stream capture);
// while every remembered use is still in flight the list simply grows -- there is no cap that could drop a live one.
int ws_release(spart_ctx* ctx, const char* base, size_t bytes, hipStream_t st, const char* who) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
  const bool capturing = cs != hipStreamCaptureStatusNone;
  WsUse* slot = nullptr;
  for (WsUse& u : ctx->ws_uses)
    if (u.base == base && u.stream == st) slot = &u;      // same pair again: the stream orders the two uses itself
  if (!slot && ctx->ws_uses.size() >= WS_PRUNE_AT) {
    // An event query is "potentially unsafe" under a GLOBAL-mode stream capture anywhere in the process (torch.cuda.graph's
    // default): it would fail and invalidate that capture.  So: none at all while THIS stream is being captured, and
    // otherwise this thread is switched to relaxed capture interaction around the queries (what PyTorch's caching allocator
    // does around its own event queries); only events recorded outside any capture are ever queried.
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    const bool relaxed = !capturing && hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
    for (WsUse& u : ctx->ws_uses) {
      bool idle = u.captured;
      if (!idle && relaxed) {
        const hipError_t q = hipEventQuery(u.done);
        if (q == hipSuccess) idle = true;
        else (void)hipGetLastError();                     // hipErrorNotReady (or anything else): treat as in flight
      }
      if (idle) { slot = &u; break; }
    }
    if (relaxed) (void)hipThreadExchangeStreamCaptureMode(&mode);      // (back to the thread's previous mode)
    else if (!capturing) (void)hipGetLastError();
    if (slot) slot->bytes = 0;
  }
  if (!slot) {
    WsUse u;
    if (hipEventCreateWithFlags(&u.done, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      return fail(SPART_ERR_HIP, "%s: cannot create the workspace completion event", who);
    }
    ctx->ws_uses.push_back(u);
    slot = &ctx->ws_uses.back();
  }
  slot->base = base;
  slot->bytes = bytes > slot->bytes ? bytes : slot->bytes;
  slot->stream = st;
  slot->captured = capturing;
  const hipError_t e = hipEventRecord(slot->done, st);
  if (e != hipSuccess) return fail(SPART_ERR_HIP, "%s: recording the workspace completion event: %s", who, hipGetErrorString(e));
  return SPART_OK;
}

// the band kernels address 8 rows of the float64 constant block with a 32-bit byte offset (stage_constants)
constexpr int64_t SPART_MAX_BATCH = 60000000;

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

struct Workspace {
  size_t cstf_off, cstd_off, atm_off, bs_off, total;
  int64_t Bp;       // row pitch of the structure-of-arrays blocks (spart_kernels.h)
  int chunk;        // samples per workgroup of the band kernels (pick_chunk) ...
  int64_t nchunk;   // ... and the number of chunks: rows of the band-sum block
};

// the band kernels address a chunk's rows with a 32-bit byte offset per lane
bool chunk_fits_32bit(int chunk, int pitch, size_t es) {
  return (int64_t)chunk * (int64_t)pitch * (int64_t)es <= (int64_t)3900000000LL;
}

// samples per workgroup of the band kernels.  Large batches: ~8192 chunk rows (x 8 tiles = 65k workgroups over
// 256 CUs: the finer grain costs nothing per workgroup -- 17 table loads per lane against >= 120 samples -- and
// shortens the tail of the launch, 1.4 % at B = 1M against 2048 rows), so the per-chunk band sums stay <= 256 MB
// (fp32) whatever B is.  Small batches: at least min(32, B/256) samples per workgroup so that the table loads are
// amortised while ~2000 workgroups remain.
int forced_chunk() {
  static const int forced = [] { const char* e = std::getenv("SPART_CHUNK"); return e ? std::atoi(e) : 0; }();   // tuning knob
  return forced;
}
int pick_chunk(int64_t B) {
  if (const int forced = forced_chunk(); forced > 0) return forced;
  int64_t c = (B + 8191) / 8192;
  int64_t small = (B + 255) / 256;
  if (small > 32) small = 32;
  if (c < small) c = small;
  return (int)(c < 1 ? 1 : c);
}

Workspace carve(int dtype, int64_t B) {
  size_t es = dtype == SPART_F64 ? 8 : 4;
  Workspace w;
  w.Bp = row_pitch_of(B);
  w.chunk = pick_chunk(B);
  w.nchunk = (B + w.chunk - 1) / w.chunk;
  const size_t Bp = (size_t)w.Bp;
  size_t o = 0;
  // float32 constants only in the float32 modes; the float64 constants are there in both (the default float32 mode's
  // column kernel is float64: k_columns<double, float>).  ~0.9 KB per sample.
  w.cstf_off = o; o = align_up(o + Bp * NCONST * 4);     // (float64 calls use it with spart_materialize.f32_bands)
  w.cstd_off = o; o = align_up(o + Bp * NCONST * 8);
  w.atm_off = o;  o = align_up(o + Bp * NATM * 8);
  w.bs_off = o;  o = align_up(o + (size_t)w.nchunk * (size_t)(NTILE * TILE) * 4 * es);
  w.total = o;
  return w;
}

// A bound of carve(SPART_F64, B).total over EVERY batch 1 <= B <= R (carve itself is not monotonic in B: the band-sum rows
// follow pick_chunk).  The three per-sample blocks grow with row_pitch_of(B), which is monotonic, so R bounds them.  The
// band-sum block has nchunk = ceil(B / pick_chunk(B)) rows: pick_chunk(B) >= ceil(B / 8192) >= B / 8192 gives nchunk <= 8192,
// and nchunk <= B <= R always; a forced SPART_CHUNK = c gives ceil(B / c) <= ceil(R / c).
size_t carve_bound_f64(int64_t R) {
  const Workspace w = carve(SPART_F64, R);
  const int forced = forced_chunk();
  const int64_t nmax = forced > 0 ? (R + forced - 1) / forced : std::min<int64_t>(R, 8192);
  return align_up(w.bs_off + (size_t)nmax * (size_t)(NTILE * TILE) * 4 * 8);
}

// the constants block of dtype T in a call's workspace, and the context's table of that dtype
template <typename T> T* constants(char* wsp, const Workspace& ws) { return (T*)(wsp + (sizeof(T) == 4 ? ws.cstf_off : ws.cstd_off)); }
template <typename T> const T* table(const spart_ctx* ctx) { return sizeof(T) == 4 ? (const T*)ctx->tabF : (const T*)ctx->tabD; }

template <typename T> int upload(T** dst, const std::vector<T>& src) {
  HIP_TRY(hipMalloc((void**)dst, src.size() * sizeof(T)));
  HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return SPART_OK;
}

// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a template argument
template <typename F> void with_flag(bool b, F&& f) { b ? f(std::true_type{}) : f(std::false_type{}); }

// The compiled variants of a kernel family: one list per family, in ascending order.  with(v, f) calls
// f(std::integral_constant<int, v>{}) and returns true if v is in the list; a value the list lacks launches nothing and
// the caller fails the call.
template <int... V> struct Variants {
  template <typename F> static bool with(int v, F&& f) { return ((v == V && (f(std::integral_constant<int, V>{}), true)) || ...); }
  // the smallest variant >= need (the largest if none is)
  static constexpr int at_least(int need) {
    int r = 0;
    for (int v : {V...})
      if ((r = v) >= need) break;
    return r;
  }
};

// fast: Newton LIDF / 8-point hot-spot rule (legacy float32 columns and the float32 stage-level entry points)
int launch_prelude(bool fast, ParamPtrs pp, int mask, int64_t B, int64_t Bp, float* cstF, double* cstD, double* atm,
                   hipStream_t st) {
  const bool user = pp.lidf != nullptr || (pp.nlayers > 0 && pp.nlayers != NLAYER);   // canopy state of the caller's own
  if (user && pp.nlayers <= 0) pp.nlayers = NLAYER;
  with_flag(fast, [&](auto F) {
    with_flag(user, [&](auto U) {
      hipLaunchKernelGGL((k_prelude<F, U>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, pp, mask, B, Bp, cstF, cstD, atm);
    });
  });
  HIP_TRY(hipGetLastError());
  return SPART_OK;
}

// a stage call's parameter columns: params[first + i] = p[i], every other pointer NULL
ParamPtrs param_slice(int first, const double* const* p, int n) {
  ParamPtrs pp;
  std::memset(&pp, 0, sizeof(pp));
  for (int i = 0; i < n; ++i) pp.p[first + i] = p[i];
  return pp;
}

// The full-band kernel k_bands<T, MAT, FULL, NT>.  MAT: 0 no spectra stored, 1 materialised spectra, 2 the same with the
// caller's dry-soil spectra.  FULL: 0 pruned (the stored spectra only), 1 band sums, 2 four band sums.  MAT = FULL = 0
// would do nothing and is not compiled; NT (non-temporal row stores) exists for MAT != 0 only, MAT = 0 stores no rows.
// float MAT = 0, the headline's dominant kernel, is compiled in its own translation unit with its own scheduling strategy
// (spart_bands_f32.hip, build.py: TU_FLAGS).
using BandsMat = Variants<0, 1, 2>;
template <int MAT> using BandsFull = std::conditional_t<MAT == 0, Variants<1, 2>, Variants<0, 1, 2>>;
template <typename T, int MAT, int FULL>
hipError_t launch_bands(bool nt, dim3 grid, hipStream_t st, const T* tab, const T* cst, int64_t Bp, int64_t B, int chunk,
                        const MatPtrs<T>& mp, T* bsum) {
  if constexpr (MAT == 0 && sizeof(T) == 4)
    return launch_bands_f32(FULL, grid.x, st, tab, cst, Bp, B, chunk, bsum);
  else if constexpr (MAT == 0)
    hipLaunchKernelGGL((k_bands<T, 0, FULL, false>), grid, dim3(TILE), 0, st, tab, cst, Bp, B, chunk, mp, bsum);
  else
    with_flag(nt, [&](auto NT) { hipLaunchKernelGGL((k_bands<T, MAT, FULL, NT>), grid, dim3(TILE), 0, st, tab, cst, Bp, B, chunk, mp, bsum); });
  return hipGetLastError();
}

}  // namespace

// any of the seven SRF-convolved (B, nb) outputs is asked for
static bool wants_srf(const spart_materialize* opt) {
  return opt && (opt->R_TOC_srf || opt->R_TOA_srf || opt->L_TOA_srf || opt->rso_srf || opt->rdo_srf || opt->rsd_srf || opt->rdd_srf);
}

// T = dtype of the full-band kernel (band sums, materialised spectra); TG = dtype of the column path: the prelude's
// constants and the canopy model inside the column kernel (double, except spart_materialize.f32_columns); TO = dtype
// of the (B, nb) outputs.  <double,double,double> = float64 mode; <float,double,float> = the default float32 mode;
// <float,double,double> = f32_bands; <float,float,float> = f32_columns.
// In EVERY mode the columns come from prelude -> k_columns<TG, TO>, i.e. from the <= 2 nb bands they depend on; the
// full-band kernel runs beside that on the caller's stream whenever full spectra are asked for (opt = NULL: band sums).
// centre = false (spart_refine_srf's forward call only): k_columns is not launched and R_TOC / R_TOA / L_TOA are not touched;
// the call's result is the *_srf outputs of opt alone.
template <typename T, typename TG, typename TO = T>
static int run_impl(spart_ctx* ctx, int64_t B, const double* const params[SPART_NPARAM], const double* rho_th,
                    const double* tau_th, void* R_TOC, void* R_TOA, void* L_TOA, const spart_materialize* opt, char* wsp,
                    const Workspace& ws, hipStream_t st, bool centre = true) {
  ParamPtrs pp = param_slice(0, params, NPARAM);
  pp.rho_th = rho_th;
  pp.tau_th = tau_th;
  pp.lidf = opt ? opt->lidf_in : nullptr;        // canopy.lidf / canopy.nlayers as the caller set them (sailh.py:48, 51)
  pp.nlayers = opt ? opt->nlayers : 0;
  const int64_t Bp = ws.Bp;
  float* cstF = constants<float>(wsp, ws);
  double* cstD = constants<double>(wsp, ws);
  double* atm = (double*)(wsp + ws.atm_off);
  // ---- everything that can fail on its arguments is checked BEFORE any launch (and before the side stream is forked)
  MatPtrs<T> mp;
  std::memset(&mp, 0, sizeof(mp));
  mp.pf = ctx->pf; mp.po = ctx->po;
  const bool nt = nt_ok(ctx->pf, sizeof(T)) && nt_ok(ctx->po, sizeof(T));     // both row grids on the 128-byte lines
  bool mat = false;
  if (opt) {
    mp.leaf_refl = (T*)opt->leaf_refl; mp.leaf_tran = (T*)opt->leaf_tran; mp.leaf_kchl = (T*)opt->leaf_kchl;
    mp.soil_refl = (T*)opt->soil_refl; mp.soil_dry = (T*)opt->soil_refl_dry;
    mp.rso = (T*)opt->rso; mp.rdo = (T*)opt->rdo; mp.rsd = (T*)opt->rsd; mp.rdd = (T*)opt->rdd;
    mp.rdry_in = (const T*)opt->rdry_in;
    mat = mp.leaf_refl || mp.leaf_tran || mp.leaf_kchl || mp.soil_refl || mp.soil_dry || mp.rso || mp.rdo || mp.rsd || mp.rdd;
  }
  if ((mat || mp.rdry_in) && !chunk_fits_32bit(ws.chunk, ctx->pf, sizeof(T)))
    return fail(SPART_ERR_INVALID, "batch too large for materialised spectra in one call (chunk %d rows x pitch %d)", ws.chunk, ctx->pf);
  const bool srf = wants_srf(opt);               // (refused with f32_columns by spart_run_batch)
  const bool full = !(opt && opt->prune_unused_bands);
  if (opt && opt->band_mean && !full)
    return fail(SPART_ERR_INVALID, "spart_run_batch: band_mean needs prune_unused_bands = 0");
  int rc;
  // optional per-stage timing: four events per call (before the prelude, after the prelude, after the full-band kernel,
  // after the column kernel)
  const bool prof = ctx->profile && ctx->ev_used + NEV <= ctx->ev.size();
  hipEvent_t* ev = prof ? &ctx->ev[ctx->ev_used] : nullptr;
  if (prof) HIP_TRY(hipEventRecord(ev[0], st));
  const bool four = opt && opt->band_mean;     // the four band sums are only kept apart when their means are asked for
  const bool bands = mat || full;              // the full-band kernel runs (otherwise: pruned, column kernel only)
  {
    Range r("SPART prelude (geometry, LIDF, hot spot, soil factors)");
    // legacy float32 columns (TG = float): the fast prelude; otherwise the literal one.  cstF only when a float32
    // full-band kernel (or the float32 column kernel) will read it.
    rc = launch_prelude(sizeof(TG) == 4 || (opt && opt->fast_prelude), pp, PRE_ALL, B, Bp, (sizeof(TG) == 4 || (sizeof(T) == 4 && bands)) ? cstF : nullptr,
                        sizeof(TG) == 8 ? cstD : nullptr, atm, st);
  }
  if (rc) return rc;
  Range rb("SPART bands + sensor (BSM, PROSPECT, SAILH | interp, SMAC, TOC->TOA)");
  T* bsum = (T*)(wsp + ws.bs_off);
  if (prof) HIP_TRY(hipEventRecord(ev[1], st));
  // The columns do not depend on the full-band kernel, so the column kernel runs on the context's side stream BESIDE it
  // and fills issue slots it leaves idle; the caller's stream waits for it at the end.
  SideLane* lane = bands ? lane_for(ctx, st) : nullptr;
  const bool fork = lane != nullptr;
  hipStream_t s2 = fork ? lane->side : st;
  auto columns = [&]() -> int {                // the column kernel, on s2
    if (centre) {
      hipLaunchKernelGGL((k_columns<TG, TO, TO>), dim3((unsigned)((B + 63) / 64)), dim3(64 * COL_WAVES), 0, s2, table<TG>(ctx),
                         (const TG*)constants<TG>(wsp, ws),
                         (const double*)atm, Bp, (const int*)ctx->band0, (const int*)ctx->band1, (const double*)ctx->frac,
                         (const double*)ctx->coef, (const double*)ctx->econv, ctx->nb,
                         (const TO*)(opt ? opt->rdry_in : nullptr), ctx->po, B, (TO*)R_TOC,
                         (TO*)R_TOA, (TO*)L_TOA, (TO*)(opt ? opt->rsoil : nullptr), (TO*)(opt ? opt->La : nullptr));
      HIP_TRY(hipGetLastError());
    }
    // the SRF-convolved columns: the same stream, behind k_columns (like it they read the prelude's constants and atmosphere rows)
    if constexpr (sizeof(TG) == 8) {
      if (srf) {
        hipLaunchKernelGGL((k_columns_srf<TO, TO>), dim3((unsigned)((B + 63) / 64), (unsigned)((ctx->nb + COL_WAVES - 1) / COL_WAVES)),
                           dim3(64 * COL_WAVES), 0, s2, (const double*)ctx->tabD, (const double*)cstD, (const double*)atm, Bp, (const int*)ctx->srf_deal,
                           (const int*)ctx->srf_start, (const int*)ctx->srf_ev, (const double*)ctx->srf_q,
                           (const double*)ctx->srf_Q, (const double*)ctx->coef, (const double*)ctx->econv, ctx->nb,
                           (const TO*)opt->rdry_in, ctx->po, B, (TO*)opt->R_TOC_srf, (TO*)opt->R_TOA_srf, (TO*)opt->L_TOA_srf,
                           (TO*)opt->rso_srf, (TO*)opt->rdo_srf, (TO*)opt->rsd_srf, (TO*)opt->rdd_srf);
        HIP_TRY(hipGetLastError());
      }
    }
    if (prof) HIP_TRY(hipEventRecord(ev[3], s2));
    return SPART_OK;
  };
  auto band_kernels = [&]() -> int {           // the full-band kernel (+ the batch-mean reduction), on the caller's stream
    // user dry-soil spectra select the reading variant whatever is stored: band sums and band_mean must see the same soil
    // as the columns (with M = 0 the kernel would mix the GSV soil from params[9..11], which may be NULL with rdry_in)
    const int M = mp.rdry_in ? 2 : (mat ? 1 : 0);
    const int F = !full ? 0 : (four ? 2 : 1);
    hipError_t e = hipSuccess;
    bool compiled = false;
    BandsMat::with(M, [&](auto MM) {
      compiled = BandsFull<MM>::with(F, [&](auto FF) {
        e = launch_bands<T, MM, FF>(nt, dim3(xcd_grid(ws.nchunk)), st, table<T>(ctx), constants<T>(wsp, ws), Bp, B, ws.chunk, mp, bsum);
      });
    });
    if (!compiled) return fail(SPART_ERR_INVALID, "spart_run_batch: no k_bands variant for MAT = %d, FULL = %d", M, F);
    if (e != hipSuccess) return fail(SPART_ERR_HIP, "spart_run_batch: k_bands<MAT = %d, FULL = %d>: %s", M, F, hipGetErrorString(e));
    if (prof) HIP_TRY(hipEventRecord(ev[2], st));
    if (opt && opt->band_mean) {
      hipLaunchKernelGGL((k_bandmean<T>), dim3((4 * NWLS + 255) / 256), dim3(256), 0, st, (const T*)bsum, ws.nchunk, B,
                         (T*)opt->band_mean);
      HIP_TRY(hipGetLastError());
    }
    return SPART_OK;
  };
  if (!bands) {                                // pruned: the column path alone
    if (prof) HIP_TRY(hipEventRecord(ev[2], st));
    rc = columns();
  } else if (!fork) {
    if ((rc = band_kernels()) == SPART_OK) rc = columns();
  } else {                                     // side stream first: its kernels are queued before the 65k workgroups of k_bands
    HIP_TRY(hipEventRecord(lane->fork, st));
    HIP_TRY(hipStreamWaitEvent(lane->side, lane->fork, 0));
    rc = columns();
    const int rc2 = band_kernels();
    // whatever happened after the fork, the caller's stream is ordered after the side stream's work again (and a HIP-graph
    // capture in progress gets its join): an error code is returned only after the join has been recorded
    const hipError_t ej = hipEventRecord(lane->join, lane->side);
    const hipError_t ew = ej == hipSuccess ? hipStreamWaitEvent(st, lane->join, 0) : ej;
    if (rc == SPART_OK) rc = rc2;
    if (rc == SPART_OK && ew != hipSuccess) rc = fail(SPART_ERR_HIP, "spart_run_batch: joining the side stream: %s", hipGetErrorString(ew));
  }
  if (rc) return rc;
  if (prof) {
    ctx->ev_forked.push_back(fork ? 1 : 0);
    ctx->ev_used += NEV;
  }
  return SPART_OK;
}

// ---- LUT inversion (csrc/spart_lut.h): GEMM + argmin on the matrix cores as a filter, exact direct evaluation of every
// candidate, brute-force fallback.  float32: K steps of 2 (v_mfma_f32_32x32x2_f32), KS = ceil((nb + 1) / 2) MFMAs per
// 32 x 32 comparisons, rounded up to one of the compiled variants; float64: K steps of 4 (v_mfma_f64_16x16x4_f64).
using LutKs = Variants<4, 7, 8, 11, 16>;           // k_lut_prep<float, KS, 32>, k_lut_scan_mfma<KS>, k_lut_collect_mfma<KS>
using LutKs64 = Variants<2, 4, 6, 8>;              // k_lut_prep<double, KS, 16>, k_lut_scan_mfma64<KS, lut_to64(KS)>,
                                                   // k_lut_collect_mfma64<KS, lut_to64(KS)>
using LutFallback = Variants<4, 8, 12, 16, 20, 24, 28, 32>;   // k_lut_fallback<T, N>: N = nb rounded up to a multiple of 4
static constexpr int lut_to64(int ks) { return ks <= 4 ? 8 : 4; }     // 16-observation blocks per wave (operand registers: 2 KS TO)
// workgroups = ceil(M / obs per workgroup) x nslice; slices are whole tiles
static int lut_slices(int64_t M, int64_t ntile, int obs_per_wg) {
  const int64_t mg = (M + obs_per_wg - 1) / obs_per_wg;
  int64_t n = (4096 + mg - 1) / mg;
  if (n > ntile) n = ntile;
  if (n > 1024) n = 1024;
  if (n < 1) n = 1;
  return (int)n;
}

// a workspace handed out field by field: take(bytes) is the field's offset, and the next field starts align_up later
struct Carver {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes);
    return at;
  }
};

struct LutLayout {
  int ks, to, rows, nslice, npart, kfma;
  int64_t ntile, nfb;
  size_t tiles, pc, ps, pt, centre, ctl, flags, fbc, fbi, total;
};
static LutLayout lut_layout(int dtype, int64_t B, int nb, int64_t M) {
  LutLayout L;
  const size_t es = dtype == SPART_F64 ? 8 : 4;
  if (dtype == SPART_F32) {
    L.rows = 32; L.ks = LutKs::at_least((nb + 2) / 2); L.to = LUT_TO; L.kfma = 2 * L.ks;
  } else {
    L.rows = 16; L.ks = LutKs64::at_least((nb + 4) / 4); L.to = lut_to64(L.ks); L.kfma = 4 * L.ks;      // ceil((nb + 1) / 4)
  }
  L.ntile = (B + L.rows - 1) / L.rows;
  L.nslice = lut_slices(M, L.ntile, L.rows * L.to * 4);
  L.npart = (64 / L.rows) * L.nslice;
  const int64_t mgroups = (M + 63) / 64;
  L.nfb = mgroups > (int64_t)LUT_FB_BLOCKS * 4 ? mgroups : (int64_t)LUT_FB_BLOCKS * 4;
  Carver c;
  L.tiles = c.take((size_t)L.ntile * L.ks * 64 * es);
  L.pc = c.take((size_t)L.npart * M * es);
  L.ps = c.take((size_t)L.npart * M * es);
  L.pt = c.take((size_t)L.npart * M * 4);
  L.centre = c.take(32 * es);
  L.ctl = c.take(LUT_CTL_WORDS * 8);
  L.flags = c.take((size_t)M * 4);
  L.fbc = c.take((size_t)L.nfb * 64 * es);
  L.fbi = c.take((size_t)L.nfb * 64 * 8);
  L.total = c.o;
  return L;
}
// Delta = coef_ef * [(N_a + Y) + (N_b + Y)]: spart_lut.h derives (3 nb + 2 K + 13) u; + 3 and 1 % for the second-order terms.
// coef_e: the filter's own error E = (nb + 2 K + 7) u (N + Y), with the same slack
static double lut_coef_ef(int nb, int kfma, double u) { return (3.0 * nb + 2.0 * kfma + 16.0) * 1.01 * u; }
static double lut_coef_e(int nb, int kfma, double u) { return (nb + 2.0 * kfma + 10.0) * 1.01 * u; }

template <typename T>
static int lut_impl(spart_ctx* ctx, int dtype, int64_t B, int nb, const void* lut_, int64_t M, const void* obs_,
                    const void* weights, int64_t* best_idx, void* best_cost, char* wsp, hipStream_t st) {
  const LutLayout L = lut_layout(dtype, B, nb, M);
  const T *lut = (const T*)lut_, *obs = (const T*)obs_, *w = (const T*)weights;
  T* tiles = (T*)(wsp + L.tiles);
  T* pc = (T*)(wsp + L.pc);
  T* ps = (T*)(wsp + L.ps);
  int* pt = (int*)(wsp + L.pt);
  T* centre = (T*)(wsp + L.centre);
  unsigned long long* ctl = (unsigned long long*)(wsp + L.ctl);
  int* flags = (int*)(wsp + L.flags);
  T* fbc = (T*)(wsp + L.fbc);
  int64_t* fbi = (int64_t*)(wsp + L.fbi);
  hipLaunchKernelGGL((k_lut_centre<T>), dim3(nb), dim3(256), 0, st, lut, nb, B, centre, ctl);
  HIP_TRY(hipGetLastError());
  const dim3 gprep((unsigned)((L.ntile * L.rows + 255) / 256));
  const dim3 grid((unsigned)((M + L.rows * L.to * 4 - 1) / (L.rows * L.to * 4)), (unsigned)L.nslice);
  bool compiled;
  if constexpr (sizeof(T) == 4)
    compiled = LutKs::with(L.ks, [&](auto K) {
      hipLaunchKernelGGL((k_lut_prep<float, K, 32>), gprep, dim3(256), 0, st, lut, w, (const float*)centre, nb, B, L.ntile, tiles, ctl);
      hipLaunchKernelGGL((k_lut_scan_mfma<K>), grid, dim3(256), 0, st, (const float*)tiles, obs, w, (const float*)centre, nb, L.ntile,
                         M, L.nslice, pc, ps, pt);
    });
  else
    compiled = LutKs64::with(L.ks, [&](auto K) {
      hipLaunchKernelGGL((k_lut_prep<double, K, 16>), gprep, dim3(256), 0, st, lut, w, (const double*)centre, nb, B, L.ntile, tiles, ctl);
      hipLaunchKernelGGL((k_lut_scan_mfma64<K, lut_to64(K)>), grid, dim3(256), 0, st, (const double*)tiles, obs, w,
                         (const double*)centre, nb, L.ntile, M, L.nslice, pc, ps, pt);
    });
  if (!compiled) return fail(SPART_ERR_INVALID, "spart_lut_nearest: no compiled LUT scan for KS = %d", L.ks);
  HIP_TRY(hipGetLastError());
  const T coef_ef = (T)lut_coef_ef(nb, L.kfma, (double)LutNum<T>::u), coef_e = (T)lut_coef_e(nb, L.kfma, (double)LutNum<T>::u);
  const dim3 gobs((unsigned)((M + 3) / 4));                // one wave per observation
  hipLaunchKernelGGL((k_lut_reduce_exact<T, (sizeof(T) == 4 ? 32 : 16)>), gobs, dim3(256), 0, st, (const T*)pc, (const T*)ps,
                     (const int*)pt, (const T*)tiles, L.ks, lut, obs, w, (const T*)centre, nb, B, M, L.npart, coef_e, coef_ef, ctl,
                     flags, best_idx, (T*)best_cost);
  HIP_TRY(hipGetLastError());
  // the flagged observations (normally a handful, possibly all of them for degenerate data): the grid is fixed, the
  // kernels read the count on the device, so the call stays asynchronous and graph-capturable
  const int nbc = (nb + 3) / 4 * 4;
  const size_t fb_lds = (size_t)4 * LUT_FB_ROWS * nbc * sizeof(T);
  if (!LutFallback::with(nbc, [&](auto N) {
        hipLaunchKernelGGL((k_lut_fallback<T, N>), dim3(LUT_FB_BLOCKS), dim3(256), fb_lds, st, lut, obs, w, nb, B,
                           (const T*)tiles, L.ks, (const unsigned long long*)ctl, (const int*)flags, fbc, fbi);
      }))
    return fail(SPART_ERR_INVALID, "spart_lut_nearest: no compiled LUT fallback for %d bands", nbc);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((k_lut_fallback_merge<T>), dim3(256), dim3(256), 0, st, B, LUT_FB_BLOCKS * 4, (const unsigned long long*)ctl,
                     (const int*)flags, (const T*)fbc, (const int64_t*)fbi, best_idx, (T*)best_cost);
  HIP_TRY(hipGetLastError());
  return SPART_OK;
}

// ---- LUT top-k (csrc/spart_lut.h, "top-k"): the k = 1 path's centre / prep / scan, a bound, a collecting second scan,
// an exact select per observation and a brute force for the flagged ones.  Observations go in chunks of LUT_TOPK_CHUNK.
struct LutTopkLayout {
  LutLayout base;                                  // ks, to, rows, kfma, ntile of the k = 1 layout for the same call
  int nslice, npart, nslice2, cap;
  int64_t mc;                                      // observations per chunk
  size_t tiles, pc, ps, pt, thr, cn, cand, centre, ctl, flags, total;
};
static LutTopkLayout lut_topk_layout(int dtype, int64_t B, int nb, int64_t M, int k) {
  LutTopkLayout L;
  L.base = lut_layout(dtype, B, nb, M < LUT_TOPK_CHUNK ? M : LUT_TOPK_CHUNK);
  const size_t es = dtype == SPART_F64 ? 8 : 4;
  const LutLayout& b = L.base;
  const int groups = 64 / b.rows;
  L.mc = M < LUT_TOPK_CHUNK ? M : LUT_TOPK_CHUNK;
  // the bound needs >= k finite partial values of distinct rows: at least 2k values (best + second per partial result)
  int64_t ns = b.nslice;
  const int64_t need = (2 * (int64_t)k + groups - 1) / groups;
  if (ns < need) ns = need;
  if (ns > LUT_TOPK_MAXPART / groups) ns = LUT_TOPK_MAXPART / groups;
  if (ns > b.ntile) ns = b.ntile;
  if (ns < 1) ns = 1;
  L.nslice = (int)ns;
  L.npart = groups * L.nslice;
  L.nslice2 = b.nslice;                            // the collect scan: the k = 1 scan's occupancy rule
  L.cap = lut_topk_cap(k);
  const size_t mc = (size_t)L.mc;
  Carver c;
  L.tiles = c.take((size_t)b.ntile * b.ks * 64 * es);
  L.pc = c.take((size_t)L.npart * mc * es);
  L.ps = c.take((size_t)L.npart * mc * es);
  L.pt = c.take((size_t)L.npart * mc * 4);
  L.thr = c.take(mc * es);
  L.cn = c.take(mc * 4);
  L.cand = c.take(mc * (size_t)L.cap * 4);
  L.centre = c.take(32 * es);
  L.ctl = c.take(LUT_TOPK_CTL_WORDS * 8);
  L.flags = c.take((size_t)M * 4);
  L.total = c.o;
  return L;
}

template <typename T>
static int lut_topk_impl(int dtype, int64_t B, int nb, const void* lut_, int64_t M, const void* obs_, const void* weights, int k,
                         int64_t* idx, void* cost, char* wsp, hipStream_t st) {
  const char* who = "spart_lut_topk";
  const LutTopkLayout L = lut_topk_layout(dtype, B, nb, M, k);
  const LutLayout& b = L.base;
  constexpr int ROWS = sizeof(T) == 4 ? 32 : 16;
  const T *lut = (const T*)lut_, *obs = (const T*)obs_, *w = (const T*)weights;
  T* tiles = (T*)(wsp + L.tiles);
  T* pc = (T*)(wsp + L.pc);
  T* ps = (T*)(wsp + L.ps);
  int* pt = (int*)(wsp + L.pt);
  T* thr = (T*)(wsp + L.thr);
  int* cn = (int*)(wsp + L.cn);
  int* cand = (int*)(wsp + L.cand);
  T* centre = (T*)(wsp + L.centre);
  unsigned long long* ctl = (unsigned long long*)(wsp + L.ctl);
  int* flags = (int*)(wsp + L.flags);
  HIP_TRY(hipMemsetAsync(ctl, 0, LUT_TOPK_CTL_WORDS * 8, st));
  hipLaunchKernelGGL((k_lut_centre<T>), dim3(nb), dim3(256), 0, st, lut, nb, B, centre, ctl);
  HIP_TRY(hipGetLastError());
  const dim3 gprep((unsigned)((b.ntile * b.rows + 255) / 256));
  const int opw = b.rows * b.to * 4;                 // observations per scan workgroup
  bool compiled;
  if constexpr (sizeof(T) == 4)
    compiled = LutKs::with(b.ks, [&](auto K) {
      hipLaunchKernelGGL((k_lut_prep<float, K, 32>), gprep, dim3(256), 0, st, lut, w, (const float*)centre, nb, B, b.ntile, tiles, ctl);
    });
  else
    compiled = LutKs64::with(b.ks, [&](auto K) {
      hipLaunchKernelGGL((k_lut_prep<double, K, 16>), gprep, dim3(256), 0, st, lut, w, (const double*)centre, nb, B, b.ntile, tiles, ctl);
    });
  if (!compiled) return fail(SPART_ERR_INVALID, "%s: no compiled LUT scan for KS = %d", who, b.ks);
  HIP_TRY(hipGetLastError());
  const T coef_ef = (T)lut_coef_ef(nb, b.kfma, (double)LutNum<T>::u);
  for (int64_t m0 = 0; m0 < M; m0 += L.mc) {
    const int64_t mc = M - m0 < L.mc ? M - m0 : L.mc;
    const T* ob = obs + m0 * nb;
    const unsigned gx = (unsigned)((mc + opw - 1) / opw);
    const dim3 g1(gx, (unsigned)L.nslice), g2(gx, (unsigned)L.nslice2), gobs((unsigned)((mc + 3) / 4));
    auto bound = [&] {
      hipLaunchKernelGGL((k_lut_topk_bound<T>), gobs, dim3(256), 0, st, (const T*)pc, (const T*)ps, ob, w, (const T*)centre, nb, mc,
                         L.npart, k, coef_ef, (const unsigned long long*)ctl, thr, cn);
    };
    if constexpr (sizeof(T) == 4)
      LutKs::with(b.ks, [&](auto K) {
        hipLaunchKernelGGL((k_lut_scan_mfma<K>), g1, dim3(256), 0, st, (const float*)tiles, ob, w, (const float*)centre, nb, b.ntile,
                           mc, L.nslice, pc, ps, pt);
        bound();
        hipLaunchKernelGGL((k_lut_collect_mfma<K>), g2, dim3(256), 0, st, (const float*)tiles, ob, w, (const float*)centre, nb,
                           b.ntile, mc, L.nslice2, (const float*)thr, L.cap, cn, cand);
      });
    else
      LutKs64::with(b.ks, [&](auto K) {
        hipLaunchKernelGGL((k_lut_scan_mfma64<K, lut_to64(K)>), g1, dim3(256), 0, st, (const double*)tiles, ob, w,
                           (const double*)centre, nb, b.ntile, mc, L.nslice, pc, ps, pt);
        bound();
        hipLaunchKernelGGL((k_lut_collect_mfma64<K, lut_to64(K)>), g2, dim3(256), 0, st, (const double*)tiles, ob, w,
                           (const double*)centre, nb, b.ntile, mc, L.nslice2, (const double*)thr, L.cap, cn, cand);
      });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_lut_topk_select<T, ROWS, false>), gobs, dim3(256), 0, st, lut, obs, w, nb, B, (const T*)tiles, b.ks, m0, mc,
                       k, (const T*)thr, (const int*)cn, (const int*)cand, L.cap, ctl, flags, idx, (T*)cost);
    HIP_TRY(hipGetLastError());
  }
  // the flagged observations of every chunk (fixed grid; the kernel reads the count on the device)
  hipLaunchKernelGGL((k_lut_topk_select<T, ROWS, true>), dim3(LUT_FB_BLOCKS), dim3(256), 0, st, lut, obs, w, nb, B,
                     (const T*)tiles, b.ks, (int64_t)0, M, k, (const T*)nullptr, (const int*)nullptr, (const int*)nullptr, L.cap, ctl,
                     flags, idx, (T*)cost);
  HIP_TRY(hipGetLastError());
  return SPART_OK;
}

// ---- wide LUT top-k (csrc/spart_lut.h, "wide top-k"): any 1 <= nb <= SPART_NWLS, K streamed through LDS.
struct LutWideLayout {
  int rows, nbp, nch, nslice, nslice2, npart, cap;
  int64_t mc, gx;                                  // observations per chunk, observation blocks of a full chunk
  size_t centre, norm, ctl, bq, ya, pc, ps, thr, cn, cand, flags, q, total;
};
// obsw = true: spart_lut_topk_obs_weights -- Bq holds 2 nbp entries per observation, the chunk is cut so that Bq stays
// within LUTOW_BQ_BYTES, ya holds (Y, Nbound) in float64, q the per-band Q_j, and the ctl words gain Nmax of the norm pass
static LutWideLayout lut_wide_layout(int dtype, int64_t B, int nb, int64_t M, int k, bool obsw) {
  LutWideLayout L;
  const size_t es = dtype == SPART_F64 ? 8 : 4;
  L.rows = dtype == SPART_F64 ? 16 : 32;
  const int groups = 64 / L.rows;
  const int64_t owg = 2 * LUTW_TB * L.rows, rwg = 2 * LUTW_TR * L.rows;
  const int64_t nrb = (B + rwg - 1) / rwg;
  L.nbp = (nb + 1 + LUTW_KC - 1) / LUTW_KC * LUTW_KC;        // K = nb + 1 (the n_b column), whole chunks
  int64_t chunk = LUTW_CHUNK;
  if (obsw) {
    const int64_t fit = (int64_t)(LUTOW_BQ_BYTES / (2 * (size_t)L.nbp * es)) / 1024 * 1024;
    chunk = fit < 1024 ? 1024 : (fit < chunk ? fit : chunk);
  }
  L.mc = M < chunk ? M : chunk;
  L.gx = (L.mc + owg - 1) / owg;
  L.nch = L.nbp / LUTW_KC;
  // slices: enough workgroups to fill the device (~2048), and for the bound at least 2k values (two per partial result)
  int64_t occ = (2048 + L.gx - 1) / L.gx;
  const int64_t need = (2 * (int64_t)k + 2 * groups - 1) / (2 * groups);
  int64_t ns = occ > need ? occ : need;
  if (ns > LUT_TOPK_MAXPART / (2 * groups)) ns = LUT_TOPK_MAXPART / (2 * groups);
  if (ns > nrb) ns = nrb;
  if (ns < 1) ns = 1;
  L.nslice = (int)ns;
  L.npart = 2 * groups * L.nslice;
  if (occ > nrb) occ = nrb;
  if (occ > 65535) occ = 65535;
  L.nslice2 = (int)(occ < 1 ? 1 : occ);
  L.cap = lut_topk_cap(k);
  const size_t mc = (size_t)L.mc;
  Carver c;
  L.centre = c.take((size_t)nb * es);
  L.norm = c.take((size_t)B * es);
  L.ctl = c.take((obsw ? 2 * LUT_TOPK_CTL_WORDS : LUT_TOPK_CTL_WORDS) * 8);
  L.bq = c.take(mc * (size_t)L.nbp * es * (obsw ? 2 : 1));
  L.ya = c.take(mc * (obsw ? 16 : es));
  L.pc = c.take((size_t)L.npart * mc * es);
  L.ps = c.take((size_t)L.npart * mc * es);
  L.thr = c.take(mc * es);
  L.cn = c.take(mc * 4);
  L.cand = c.take(mc * (size_t)L.cap * 4);
  L.flags = c.take((size_t)M * 4);
  L.q = c.take(obsw ? (size_t)nb * 8 : 0);
  L.total = c.o;
  return L;
}

// The exact top-k over the candidate rows (brute = false: the chunk m0 .. m0 + mc) and over every row for the flagged
// observations (brute = true, after the last chunk): the consumer of lut_wide_impl for the two wide top-k searches
template <typename T, bool OBSW>
static auto lutw_topk_consumer(const T* lut, const T* obs, const T* w, int nb, int64_t B, int64_t M, int k, int64_t* idx, void* cost) {
  return [=](bool brute, int64_t m0, int64_t mc, const LutWideLayout& L, char* wsp, hipStream_t st) {
    constexpr int ROWS = LutWide<T>::ROWS;
    const size_t sel_lds = (size_t)LUT_TOPK_BUF * 12 + 2 * (size_t)nb * sizeof(T);
    unsigned long long* ctl = (unsigned long long*)(wsp + L.ctl);
    int* flags = (int*)(wsp + L.flags);
    const T* norm = (const T*)(wsp + L.norm);
    if (!brute)
      hipLaunchKernelGGL((k_lutw_select<T, ROWS, false, OBSW>), dim3((unsigned)mc), dim3(64), sel_lds, st, lut, obs, w, nb, B, m0, mc,
                         k, (const T*)(wsp + L.thr), (const int*)(wsp + L.cn), (const int*)(wsp + L.cand), L.cap, ctl, flags, idx,
                         (T*)cost, norm);
    else   // (fixed grid; the kernel reads the count on the device)
      hipLaunchKernelGGL((k_lutw_select<T, ROWS, true, OBSW>), dim3(LUTW_SELECT_BLOCKS), dim3(64), sel_lds, st, lut, obs, w, nb, B,
                         (int64_t)0, M, k, (const T*)nullptr, (const int*)nullptr, (const int*)nullptr, L.cap, ctl, flags, idx,
                         (T*)cost, norm);
    return SPART_OK;
  };
}

// OBSW: per-observation weights (csrc/spart_lut.h, "per-observation weights") -- the same pipeline with K = 2 nbp: its own
// observation pass, GEMM and bound, a per-band pass k_lutow_q before the chunks, and the consumer's OBSW flag.
// kcap sizes the layout (the candidate capacity is lut_topk_cap(kcap) tiles); U is the kth smallest partial value and the
// threshold admits every row within `cut` of the kth best (OBSW only; the top-k searches pass kcap = kth = k and cut = 0.0).
// filter = false queues the row pass only (centres and norms), no GEMM: a consumer that flags every observation itself.
// consume(brute, m0, mc, layout, workspace, stream) queues what reads the candidate lists: once per chunk with brute =
// false, and once after the last chunk with brute = true for the flagged observations of every chunk.
template <typename T, bool OBSW, typename Consume>
static int lut_wide_impl(int dtype, int64_t B, int nb, const void* lut_, int64_t M, const void* obs_, const void* weights, int kcap,
                         int kth, double cut, bool filter, char* wsp, hipStream_t st, Consume&& consume) {
  const LutWideLayout L = lut_wide_layout(dtype, B, nb, M, kcap, OBSW);
  constexpr int ROWS = LutWide<T>::ROWS;
  constexpr int OWG = 2 * LUTW_TB * ROWS;
  constexpr auto gemm_scan = OBSW ? k_lutow_gemm<T, false> : k_lutw_gemm<T, false>;
  constexpr auto gemm_collect = OBSW ? k_lutow_gemm<T, true> : k_lutw_gemm<T, true>;
  const T *lut = (const T*)lut_, *obs = (const T*)obs_, *w = (const T*)weights;
  T* centre = (T*)(wsp + L.centre);
  T* norm = (T*)(wsp + L.norm);
  unsigned long long* ctl = (unsigned long long*)(wsp + L.ctl);
  T* bq = (T*)(wsp + L.bq);
  void* ya = wsp + L.ya;                               // Y in the dtype; OBSW: (Y, Nbound) in float64
  T* pc = (T*)(wsp + L.pc);
  T* ps = (T*)(wsp + L.ps);
  T* thr = (T*)(wsp + L.thr);
  int* cn = (int*)(wsp + L.cn);
  int* cand = (int*)(wsp + L.cand);
  unsigned long long* qb = (unsigned long long*)(wsp + L.q);       // OBSW only: the per-band Q_j
  // the coefficients of Delta (spart_lut.h, wide top-k and per-observation weights), with the 1 % slack
  const double u = (double)LutNum<T>::u;
  const double h = (OBSW ? 2.0 * LUTW_KC : LUTW_KC) + L.nch + 1.0;
  const double ce = (4.0 + (OBSW ? 1.0 : sizeof(T) == 4 ? 1.01 : nb + 2.0) + 1.0 + 2.0 * h) * 1.01 * u;
  const double cf = 2.01 * (nb + 3.0) * 1.01 * u;
  const double cw = 2.0 * (2.0 * nb + 6.0) * 1.01 * u;             // (the shared-weights bound only)
  HIP_TRY(hipMemsetAsync(ctl, 0, (OBSW ? 2 : 1) * LUT_TOPK_CTL_WORDS * 8, st));
  if constexpr (OBSW) HIP_TRY(hipMemsetAsync(qb, 0, (size_t)nb * 8, st));
  hipLaunchKernelGGL((k_lut_centre<T>), dim3(nb), dim3(256), 0, st, lut, nb, B, centre, ctl);
  HIP_TRY(hipGetLastError());
  // OBSW: the row rule without weights; its Nmax goes to a word of its own (ctl[0] is the largest Nbound_m)
  hipLaunchKernelGGL((k_lutw_norm<T>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, lut, OBSW ? (const T*)nullptr : w,
                     (const T*)centre, nb, B, norm, ctl + (OBSW ? LUT_TOPK_CTL_WORDS : 0));
  HIP_TRY(hipGetLastError());
  if constexpr (OBSW) {
    if (filter) {
      const int64_t qy = (B + 3) / 4;
      hipLaunchKernelGGL((k_lutow_q<T>), dim3((unsigned)((nb + 63) / 64), (unsigned)(qy < 1024 ? qy : 1024)), dim3(256), 0, st, lut,
                         (const T*)norm, (const T*)centre, nb, B, qb);
      HIP_TRY(hipGetLastError());
    }
  }
  for (int64_t m0 = 0; m0 < M; m0 += L.mc) {
    const int64_t mc = M - m0 < L.mc ? M - m0 : L.mc;
    const T* ob = obs + m0 * nb;
    const unsigned gx = (unsigned)((mc + OWG - 1) / OWG), gobs = (unsigned)((mc + 3) / 4);
    if (filter) {
      if constexpr (OBSW)
        hipLaunchKernelGGL((k_lutow_obs<T>), dim3(gobs), dim3(256), 0, st, ob, w + m0 * nb, (const T*)centre,
                           (const unsigned long long*)qb, nb, L.nbp, mc, bq, (double*)ya, ctl);
      else
        hipLaunchKernelGGL((k_lutw_obs<T>), dim3(gobs), dim3(256), 0, st, ob, w, (const T*)centre, nb, L.nbp, mc, bq, (T*)ya);
      hipLaunchKernelGGL(gemm_scan, dim3(gx, (unsigned)L.nslice), dim3(256), 0, st, lut, (const T*)norm, (const T*)centre, nb, B,
                         (const T*)bq, L.nbp, mc, L.nslice, pc, ps, (const T*)nullptr, 0, (int*)nullptr, (int*)nullptr);
      if constexpr (OBSW)
        hipLaunchKernelGGL((k_lutow_bound<T>), dim3(gobs), dim3(256), 0, st, (const T*)pc, (const T*)ps, (const double*)ya, nb, mc,
                           L.npart, kth, ce, cf, cut, thr, cn);
      else
        hipLaunchKernelGGL((k_lutw_bound<T>), dim3(gobs), dim3(256), 0, st, (const T*)pc, (const T*)ps, (const T*)ya, w, nb, mc,
                           L.npart, kth, ce, cf, cw, (const unsigned long long*)ctl, thr, cn);
      hipLaunchKernelGGL(gemm_collect, dim3(gx, (unsigned)L.nslice2), dim3(256), 0, st, lut, (const T*)norm, (const T*)centre, nb, B,
                         (const T*)bq, L.nbp, mc, L.nslice2, (T*)nullptr, (T*)nullptr, (const T*)thr, L.cap, cn, cand);
    }
    const int rc = consume(false, m0, mc, L, wsp, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
  }
  const int rc = consume(true, (int64_t)0, M, L, wsp, st);             // the flagged observations of every chunk
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return SPART_OK;
}

// spart_lut_bayes once its arguments are checked (csrc/spart_lut.h, "likelihood-weighted posterior"): the per-observation-
// weights pipeline with k = 1 and the radius threshold, k_lut_bayes as its consumer.  opt->brute_force skips the filter.
template <typename T>
static int lut_bayes_impl(int dtype, int64_t B, int nb, const void* lut_, int P, const double* params, int64_t M, const void* obs_,
                          const void* weights, const spart_lut_bayes_opt& opt, const LutBayesOut& out, char* wsp, hipStream_t st) {
  constexpr int ROWS = LutWide<T>::ROWS;
  const T *lut = (const T*)lut_, *obs = (const T*)obs_, *w = (const T*)weights;
  const double two_tau = 2.0 * (opt.temperature == 0.0 ? 1.0 : opt.temperature);
  const double cut = opt.cut;
  const int force = opt.brute_force;
  const size_t lds = lut_bayes_lds_bytes(nb, sizeof(T));
  return lut_wide_impl<T, true>(
      dtype, B, nb, lut_, M, obs_, weights, LUT_BAYES_CAPK, 1, cut * (1.0 + 0x1p-50), force == 0, wsp, st,
      [=](bool brute, int64_t m0, int64_t mc, const LutWideLayout& L, char* ws, hipStream_t s) {
        unsigned long long* ctl = (unsigned long long*)(ws + L.ctl);
        int* flags = (int*)(ws + L.flags);
        const T* norm = (const T*)(ws + L.norm);
        if (!brute)
          hipLaunchKernelGGL((k_lut_bayes<T, ROWS, false>), dim3((unsigned)mc), dim3(64), lds, s, lut, obs, w, norm, params, nb, B, P,
                             m0, mc, cut, two_tau, force, (const T*)(ws + L.thr), (const int*)(ws + L.cn),
                             (const int*)(ws + L.cand), L.cap, ctl, flags, out);
        else
          hipLaunchKernelGGL((k_lut_bayes<T, ROWS, true>), dim3(LUTW_SELECT_BLOCKS), dim3(64), lds, s, lut, obs, w, norm, params, nb,
                             B, P, (int64_t)0, M, cut, two_tau, force, (const T*)nullptr, (const int*)nullptr, (const int*)nullptr,
                             L.cap, ctl, flags, out);
        return SPART_OK;
      });
}

// spart_lut_bayes_quantiles once its arguments are checked: lut_bayes_impl's pipeline and launches, with k_lut_posterior_quant
// (csrc/spart_lut.h, "weighted quantiles of the posterior") queued behind every k_lut_bayes over the same chunk or flag list.
template <typename T>
static int lut_bayes_quant_impl(int dtype, int64_t B, int nb, const void* lut_, int P, const double* params, int64_t M,
                                const void* obs_, const void* weights, const spart_lut_bayes_opt& opt, const LutBayesOut& out,
                                const LutBayesLevels& lv, double* quant, char* wsp, hipStream_t st) {
  constexpr int ROWS = LutWide<T>::ROWS;
  const T *lut = (const T*)lut_, *obs = (const T*)obs_, *w = (const T*)weights;
  const double two_tau = 2.0 * (opt.temperature == 0.0 ? 1.0 : opt.temperature);
  const double cut = opt.cut;
  const int force = opt.brute_force;
  const size_t lds = lut_bayes_lds_bytes(nb, sizeof(T));
  return lut_wide_impl<T, true>(
      dtype, B, nb, lut_, M, obs_, weights, LUT_BAYES_CAPK, 1, cut * (1.0 + 0x1p-50), force == 0, wsp, st,
      [=](bool brute, int64_t m0, int64_t mc, const LutWideLayout& L, char* ws, hipStream_t s) {
        unsigned long long* ctl = (unsigned long long*)(ws + L.ctl);
        int* flags = (int*)(ws + L.flags);
        const T* norm = (const T*)(ws + L.norm);
        if (!brute) {
          hipLaunchKernelGGL((k_lut_bayes<T, ROWS, false>), dim3((unsigned)mc), dim3(64), lds, s, lut, obs, w, norm, params, nb, B, P,
                             m0, mc, cut, two_tau, force, (const T*)(ws + L.thr), (const int*)(ws + L.cn),
                             (const int*)(ws + L.cand), L.cap, ctl, flags, out);
          HIP_TRY(hipGetLastError());
          hipLaunchKernelGGL((k_lut_posterior_quant<T, ROWS, false>), dim3((unsigned)mc), dim3(64), lds, s, lut, obs, w, norm, params, nb,
                             B, P, m0, mc, cut, two_tau, force, (const T*)(ws + L.thr), (const int*)(ws + L.cn),
                             (const int*)(ws + L.cand), L.cap, (const unsigned long long*)ctl, (const int*)flags, lv, quant);
        } else {
          hipLaunchKernelGGL((k_lut_bayes<T, ROWS, true>), dim3(LUTW_SELECT_BLOCKS), dim3(64), lds, s, lut, obs, w, norm, params, nb,
                             B, P, (int64_t)0, M, cut, two_tau, force, (const T*)nullptr, (const int*)nullptr, (const int*)nullptr,
                             L.cap, ctl, flags, out);
          HIP_TRY(hipGetLastError());
          hipLaunchKernelGGL((k_lut_posterior_quant<T, ROWS, true>), dim3(LUTW_SELECT_BLOCKS), dim3(64), lds, s, lut, obs, w, norm,
                             params, nb, B, P, (int64_t)0, M, cut, two_tau, force, (const T*)nullptr, (const int*)nullptr,
                             (const int*)nullptr, L.cap, (const unsigned long long*)ctl, (const int*)flags, lv, quant);
        }
        return SPART_OK;
      });
}

// The checks every batched entry point over B samples starts with, in this order (the LUT searches have lut_search's).
// B == 0 passes them: the caller has nothing to do.  Otherwise `ws` is the layout of the call's workspace.
static int gate(const spart_ctx* ctx, const char* who, int dtype, int64_t B, const void* workspace, size_t workspace_bytes,
                Workspace& ws) {
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (B > SPART_MAX_BATCH) return fail(SPART_ERR_INVALID, "%s: at most %lld samples per call", who, (long long)SPART_MAX_BATCH);
  if (dtype != SPART_F32 && dtype != SPART_F64) return fail(SPART_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  if (B < 0) return fail(SPART_ERR_INVALID, "%s: negative batch", who);
  if (B == 0) return SPART_OK;
  ws = carve(dtype, B);
  if (!workspace || workspace_bytes < ws.total)
    return fail(SPART_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, ws.total, workspace_bytes);
  return SPART_OK;
}

// Which parameter columns may be NULL (the counterpart of spart_amd.engine.NULLABLE): B, lat, lon (params 9-11) with user
// dry-soil spectra, LIDFa, LIDFb (16, 17) with a given lidf.  The soil of spart_bsm_batch is params 9-14, the canopy of
// spart_sailh_batch params 15-18.
static bool may_be_null(int param, bool rdry, bool lidf) {
  return (rdry && param >= 9 && param <= 11) || (lidf && (param == 16 || param == 17));
}
// the index of the first NULL pointer of p[0 .. n), or n
template <typename P> static int first_null(const P* p, int n) {
  int i = 0;
  while (i < n && p[i]) ++i;
  return i;
}

// f(float{}) or f(double{}) for a call's dtype
template <typename F> static int by_dtype(int dtype, F&& f) { return dtype == SPART_F32 ? f(float{}) : f(double{}); }

// select the context's device, lock the context, order the call after other streams' use of the workspace, run
// body(stream) (the launches), record the workspace's completion event -- also after a failed body: some of its kernels
// may already be queued
template <typename F>
static int guarded(spart_ctx* ctx, const char* who, const void* wsp, size_t bytes, void* stream, F&& body) {
  DeviceGuard guard(ctx->device);
  const hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(ctx->mu);
  int rc = ws_acquire(ctx, (const char*)wsp, bytes, st, who);
  if (rc) return rc;
  rc = body(st);
  char keep[512];
  if (rc) std::snprintf(keep, sizeof(keep), "%s", g_err);
  const int rc2 = ws_release(ctx, (const char*)wsp, bytes, st, who);
  if (rc) std::snprintf(g_err, sizeof(g_err), "%s", keep);
  return rc ? rc : rc2;
}

// A stage-level call (spart_prospect_batch, _bsm_, _sailh_) once its arguments are checked: the 32-bit row offsets of a
// chunk at `pitch` are checked, the prelude writes the `mask` part of the constants in the call's dtype T, then
// launch(T{}, nt, st, tab, cst) queues the stage's own kernel (nt: std::true_type when the rows at `pitch` lie on the
// 128-byte lines, the stores' NT).
template <typename L>
static int stage_call(spart_ctx* ctx, const char* who, int dtype, int64_t B, const ParamPtrs& pp, int mask, int pitch,
                      void* workspace, const Workspace& ws, void* stream, L&& launch) {
  return guarded(ctx, who, workspace, ws.total, stream, [&](hipStream_t st) {
    return by_dtype(dtype, [&](auto t) -> int {
      using T = decltype(t);
      if (!chunk_fits_32bit(ws.chunk, pitch, sizeof(T))) return fail(SPART_ERR_INVALID, "batch too large for one call");
      T* cst = constants<T>((char*)workspace, ws);
      int rc = launch_prelude(sizeof(T) == 4, pp, mask, B, ws.Bp, sizeof(T) == 4 ? (float*)cst : nullptr,
                              sizeof(T) == 8 ? (double*)cst : nullptr, nullptr, st);
      if (rc) return rc;
      with_flag(nt_ok(pitch, sizeof(T)), [&](auto nt) { launch(t, nt, st, table<T>(ctx), (const T*)cst); });
      HIP_TRY(hipGetLastError());
      return SPART_OK;
    });
  });
}

// ---- the four LUT searches: what differs between their entry points
struct LutCall {
  const char* who;
  int nb_max;               // the widest LUT the search takes
  bool has_k;               // top-k: 1 <= k <= LUT_TOPK_MAXK (spart_lut_nearest has no k)
  bool weights_required;    // weights (M, nb) may not be NULL
  bool nb_ok(int nb) const { return nb >= 1 && nb <= nb_max; }
  bool k_ok(int k) const { return !has_k || (k >= 1 && k <= LUT_TOPK_MAXK); }
};
constexpr LutCall LUT_NEAREST = {"spart_lut_nearest", 31, false, false};
constexpr LutCall LUT_TOPK = {"spart_lut_topk", 31, true, false};
constexpr LutCall LUT_WIDE = {"spart_lut_topk_wide", NWLS, true, false};
constexpr LutCall LUT_OBSW = {"spart_lut_topk_obs_weights", NWLS, true, true};

static bool dtype_ok(int dtype) { return dtype == SPART_F32 || dtype == SPART_F64; }

// The sizes a search has a workspace for: every *_workspace_bytes is its layout's total when this holds and 0 otherwise,
// and the *_stats calls take that 0 as their size check.  (lut_search also refuses B or M above 2e9.)
static bool lut_sizes_ok(const LutCall& c, int dtype, int64_t B, int nb, int64_t M, int k) {
  return B > 0 && M > 0 && c.nb_ok(nb) && c.k_ok(k) && dtype_ok(dtype);
}

// A LUT search from its entry point: the argument checks, in this order, then impl(T{}, workspace, stream) (the launches)
// under guarded().  M == 0 passes the checks with nothing to do.  `need` is the search's own *_workspace_bytes.
template <typename F>
static int lut_search(spart_ctx* ctx, const LutCall& c, int dtype, int64_t B, int nb, const void* lut, int64_t M, const void* obs,
                      const void* weights, int k, const void* idx, const void* cost, void* workspace, size_t workspace_bytes,
                      size_t need, void* stream, F&& impl) {
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", c.who);
  if (!dtype_ok(dtype)) return fail(SPART_ERR_INVALID, "%s: bad dtype %d", c.who, dtype);
  if (B < 0 || M < 0 || !c.nb_ok(nb) || B > 2000000000LL || M > 2000000000LL)
    // (two wordings of the nb range, as the narrow and the wide searches have always reported it)
    return fail(SPART_ERR_INVALID, c.nb_max == 31 ? "%s: bad sizes (B=%lld M=%lld nb=%d; nb <= %d, B and M <= 2e9)"
                                                  : "%s: bad sizes (B=%lld M=%lld nb=%d; 1 <= nb <= %d, B and M <= 2e9)",
                c.who, (long long)B, (long long)M, nb, c.nb_max);
  if (!c.k_ok(k)) return fail(SPART_ERR_INVALID, "%s: k = %d, expected 1 <= k <= %d", c.who, k, LUT_TOPK_MAXK);
  if (M == 0) return SPART_OK;
  if (B == 0) return fail(SPART_ERR_INVALID, "%s: empty LUT", c.who);
  if (!lut || !obs || !idx || !cost || (c.weights_required && !weights)) return fail(SPART_ERR_INVALID, "%s: null argument", c.who);
  if (!workspace || workspace_bytes < need)
    return fail(SPART_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", c.who, need, workspace_bytes);
  return guarded(ctx, c.who, workspace, need, stream,
                 [&](hipStream_t st) { return by_dtype(dtype, [&](auto t) { return impl(t, (char*)workspace, st); }); });
}

// The control words of the last search that used `workspace`, for its *_stats call `who`: word 0 is the scale of the
// rounding bound as a bit pattern in the search's dtype, words 1 .. ncount are counters.  Only the search's own words are
// read (the k = 1 layout reserves LUT_CTL_WORDS).  sizes_ok: the search's *_workspace_bytes is not 0; only then is
// ctl_offset() -- the offset of the words in the search's layout -- evaluated.
template <typename F>
static int lut_read_stats(spart_ctx* ctx, const char* who, int dtype, const void* workspace, bool sizes_ok, F&& ctl_offset,
                          int64_t* const* counts, int ncount, double* scale) {
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (!workspace || first_null(counts, ncount) < ncount || !scale || !sizes_ok)
    return fail(SPART_ERR_INVALID, "%s: bad argument", who);
  DeviceGuard guard(ctx->device);
  unsigned long long ctl[LUT_TOPK_CTL_WORDS];
  HIP_TRY(hipMemcpy(ctl, (const char*)workspace + ctl_offset(), (size_t)(1 + ncount) * 8, hipMemcpyDeviceToHost));
  for (int i = 0; i < ncount; ++i) *counts[i] = (int64_t)ctl[1 + i];
  if (dtype == SPART_F32) {
    const unsigned b = (unsigned)ctl[0];
    float f;
    std::memcpy(&f, &b, 4);
    *scale = f;
  } else {
    std::memcpy(scale, &ctl[0], 8);
  }
  return SPART_OK;
}
static_assert(LUT_CTL_WORDS <= LUT_TOPK_CTL_WORDS, "lut_read_stats: the buffer holds either search's control words");

// spart_lut_summarise once its arguments are checked: one launch of single-wave workgroups, no workspace.  Only a launch
// above LUT_SUM_SMALL_K can ask for more dynamic LDS than the 64 KiB a kernel gets without opting in.
static int launch_lut_summarise(int64_t B, int P, const double* params, int64_t M, int k, const int64_t* idx, double* mean,
                                double* median, double* sdev, int32_t* count, hipStream_t st) {
  const int G = lut_sum_group(P, k);
  const size_t lds = lut_sum_lds_bytes(P, k);
  if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)k_lut_summarise, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t items = (M + G - 1) / G;
  const unsigned blocks = (unsigned)(items < LUT_SUM_MAX_BLOCKS ? items : LUT_SUM_MAX_BLOCKS);
  hipLaunchKernelGGL(k_lut_summarise, dim3(blocks), dim3(64), lds, st, params, B, P, idx, M, k, G, mean, median, sdev, count);
  HIP_TRY(hipGetLastError());
  return SPART_OK;
}

// ---- The refinement family (csrc/spart_refine.h, spart_refine_views.h, spart_refine_mix.h, spart_refine_posterior.h):
// spart_refine, spart_refine_srf, spart_refine_posterior, spart_refine_views and spart_refine_mix share one workspace layout, one
// chunk loop and one entry check.  A call fits n unknowns per observation from V views (or mixture components) of it, F free
// columns each, the first Fs of them shared by the views; the single-view entries are {1, F, F, F}.  The forward block
// (ForwardBlock), the forward call (Forward), the size guard (fit_sizes_ok), the check of the free columns (refine_check_fit)
// and the tail of an entry (fit_tail) also serve the tiles, the series, Sobol' and the sampler further down.
struct RefineShape {
  int V, F, Fs, n;
};

// What every *_workspace_bytes of the family (tiles, series, Sobol' and the sampler included) asks of ctx, M and F before its own
static bool fit_sizes_ok(const spart_ctx* ctx, int64_t M, int F) {
  return ctx && ctx->nb > 0 && M > 0 && M <= 2000000000LL && F >= 1 && F <= REFINE_MAXF;
}

// The forward block, the part of a workspace every entry that calls the forward model on a table has: the (27, rows)
// parameter table, the three (rows, nb) column blocks and the forward call's own workspace.  The caller sizes the latter:
// exact carve() totals where the row counts of its chunks are known, carve_bound_f64(rows) where they follow a partition.
struct ForwardBlock {
  size_t table, cols[3], fwd;
};
static ForwardBlock forward_block(Carver& c, int nb, size_t rows, size_t scratch) {
  ForwardBlock b;
  b.table = c.take((size_t)NPARAM * rows * 8);
  for (size_t& o : b.cols) o = c.take(rows * (size_t)nb * 8);
  b.fwd = c.take(scratch);
  return b;
}

// The forward call of the block's table, built once per entry call.  The band model decides what it writes into the column
// block the fit reads (`y`): k_columns' three centre columns, or the ONE *_srf output of k_columns_srf the fit is about
// (k_columns is then not launched at all).
struct Forward {
  spart_ctx* ctx;
  bool srf;
  spart_materialize mat;
  double *table, *cols[3];
  const double* y;
  char* scratch;
  Forward(spart_ctx* ctx_, char* wsp, const ForwardBlock& b, int column, bool srf_, int fast_prelude, int nlayers)
      : ctx(ctx_), srf(srf_), table((double*)(wsp + b.table)), scratch(wsp + b.fwd) {
    std::memset(&mat, 0, sizeof(mat));
    mat.prune_unused_bands = 1;
    mat.fast_prelude = fast_prelude;
    mat.nlayers = nlayers;
    for (int k = 0; k < 3; ++k) cols[k] = (double*)(wsp + b.cols[k]);
    y = cols[column];
    if (srf) (column == 0 ? mat.R_TOC_srf : column == 1 ? mat.R_TOA_srf : mat.L_TOA_srf) = cols[column];
  }
  // a table of `rows` rows, parameter p at table + p rows (no template: the float64 forward kernels are instantiated here,
  // ahead of the family's own)
  int run(int64_t rows, hipStream_t st) const {
    const double* params[SPART_NPARAM];
    for (int p = 0; p < SPART_NPARAM; ++p) params[p] = table + (int64_t)p * rows;
    return run_impl<double, double, double>(ctx, rows, params, nullptr, nullptr, cols[0], cols[1], cols[2], &mat, scratch,
                                            carve(SPART_F64, rows), st, !srf);
  }
};

// The workspace is sized by ONE chunk -- min(M, views_chunk(V, F)) observations of V (F + 1) table rows each -- whatever M
// is: the forward block, the optimiser's state per unknown and the device copy of the call's constants.
struct RefineLayout {
  int64_t mcap;                 // observations per chunk
  ForwardBlock b;
  size_t t, A, lam, na, cfg, cfg_free, total;
};
static RefineLayout refine_layout(int nb, int64_t M, int V, int F, int n) {
  RefineLayout l;
  l.mcap = std::min<int64_t>(M, views_chunk(V, F));
  const size_t mc = (size_t)l.mcap, per = (size_t)(F + 1) * V, rows = mc * per;
  // the forward call of a full chunk and of the last, shorter one (the band-sum rows of carve() follow pick_chunk, which is
  // not monotonic in the batch)
  size_t fwd = carve(SPART_F64, (int64_t)rows).total;
  if (const int64_t rest = M % l.mcap) fwd = std::max(fwd, carve(SPART_F64, rest * (int64_t)per).total);
  Carver c;
  l.b = forward_block(c, nb, rows, fwd);
  l.t = c.take(mc * n * 8);
  l.A = c.take(mc * (size_t)(refine_ntri(n) + n) * 8);
  l.lam = c.take(mc * 8);
  l.na = c.take(mc * 4);
  l.cfg = c.take(REFINE_CFG_DOUBLES * 8);
  l.cfg_free = c.take(REFINE_MAXF * 4);
  l.total = c.o;
  return l;
}

static bool refine_sizes_ok(const spart_ctx* ctx, int64_t M, int V, int F, int n_shared) {
  if (!fit_sizes_ok(ctx, M, F) || V < 1 || V > VIEWS_MAXV || n_shared < 0 || n_shared > F) return false;
  const int n = n_shared + V * (F - n_shared);
  return n >= 1 && n <= REFINE_MAXF;
}

// A checked call, as the chunk loops and the kernel sequences see it
struct RefineRun {
  spart_ctx* ctx;
  bool srf;                     // the forward call writes the ONE *_srf column of the fit, not k_columns' three
  int64_t M;
  RefineShape s;
  RefineCfg cfg;
  spart_refine_opt o;           // (the defaults that 0 stands for filled in)
  const double *obs, *weights;
  char* wsp;
  RefineLayout l;               // refine_loop's (the tiles and the series bring their own)
  Forward forward(const ForwardBlock& b) const { return Forward(ctx, wsp, b, o.column, srf, o.fast_prelude, o.nlayers); }
};
// the blocks of the workspace; `cols` is the column block the kernel after a forward call reads
struct RefineWs {
  double* table;
  const double* cols;
  double *t, *A, *lam, *cfg;
  int32_t *na, *cfg_free;
};

// The rows of chunk m0 of an optional array of `width` values per observation: NULL stays NULL, an array shared by all
// observations is itself
template <typename T> static T* rows_at(T* p, int64_t m0, int64_t width, bool per_obs = true) {
  return p && per_obs ? p + m0 * width : p;
}
static RefineOut rows_at(const RefineOut& o, int64_t m0, const RefineShape& s, int nb) {
  return {rows_at(o.x, m0, s.n), rows_at(o.cost, m0, 1), rows_at(o.cost0, m0, 1), rows_at(o.sdev, m0, s.n), rows_at(o.n_accept, m0, 1),
          rows_at(o.y, m0, (int64_t)s.V * nb)};
}

// The chunk loop.  Per chunk of mc observations from m0: init(w, m0, mc) launches the kernel that writes the table and the
// start state, then n_fwd times the forward call of the table's rows and after(w, m0, mc, it), the kernel that reads its
// columns.
template <typename Init, typename After>
static int refine_loop(const RefineRun& r, int n_fwd, hipStream_t st, Init&& init, After&& after) {
  const RefineLayout& l = r.l;
  const Forward fwd = r.forward(l.b);
  const RefineWs w = {fwd.table, fwd.y, (double*)(r.wsp + l.t), (double*)(r.wsp + l.A),
                      (double*)(r.wsp + l.lam), (double*)(r.wsp + l.cfg), (int32_t*)(r.wsp + l.na), (int32_t*)(r.wsp + l.cfg_free)};
  for (int64_t m0 = 0; m0 < r.M; m0 += l.mcap) {
    const int mc = (int)std::min<int64_t>(l.mcap, r.M - m0);
    const int64_t rows = (int64_t)mc * (r.s.F + 1) * r.s.V;
    init(w, m0, mc);
    HIP_TRY(hipGetLastError());
    for (int it = 0; it < n_fwd; ++it) {
      if (int rc = fwd.run(rows, st)) return rc;
      after(w, m0, mc, it);
      HIP_TRY(hipGetLastError());
    }
  }
  return SPART_OK;
}

// spart_refine / spart_refine_srf: k_refine_views_init at V = 1, then n_iter + 1 times the forward call and k_refine_step
static int refine_impl(const RefineRun& r, const RefineOut& out, hipStream_t st) {
  const spart_refine_opt& o = r.o;
  const int nb = r.ctx->nb, F = r.s.F, rows = refine_lds_rows(F + 1, F, 0), W = refine_group(rows);
  const size_t lds = refine_lds_bytes(rows, W);
  return refine_loop(
      r, o.n_iter + 1, st,
      [&](const RefineWs& w, int64_t m0, int mc) {
        hipLaunchKernelGGL(k_refine_views_init, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, st, r.cfg, r.M, m0, mc, 1, F, F,
                           o.lambda0, w.table, out.x + m0 * F, w.t, w.lam, w.na, w.cfg, w.cfg_free);
      },
      [&](const RefineWs& w, int64_t m0, int mc, int it) {
        hipLaunchKernelGGL(k_refine_step, dim3((unsigned)((mc + W - 1) / W)), dim3(64), lds, st, (const double*)w.cols,
                           r.obs + m0 * nb, rows_at(r.weights, m0, nb, o.weights_per_obs), o.weights_per_obs ? 1 : 0,
                           (const double*)w.cfg, (const int32_t*)w.cfg_free, w.table, mc, F, nb, W, it, it == o.n_iter ? 1 : 0, w.t,
                           w.A, w.lam, w.na, rows_at(out, m0, r.s, nb), rows_at(o.prior_mean, m0, F, o.prior_per_obs),
                           rows_at(o.prior_weight, m0, F, o.prior_per_obs), o.prior_per_obs ? 1 : 0);
      });
}

// spart_refine_posterior: k_refine_views_init at V = 1, ONE forward call per chunk and k_refine_posterior.  The optimiser's
// state of the layout is not used, so its A block takes the init kernel's x when the caller does not ask for it.
static int posterior_impl(const RefineRun& r, const spart_posterior_out& out, hipStream_t st) {
  const spart_refine_opt& o = r.o;
  const int nb = r.ctx->nb, F = r.s.F, W = refine_posterior_group(F);
  const size_t lds = refine_posterior_lds_bytes(F, W);
  return refine_loop(
      r, 1, st,
      [&](const RefineWs& w, int64_t m0, int mc) {
        hipLaunchKernelGGL(k_refine_views_init, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, st, r.cfg, r.M, m0, mc, 1, F, F,
                           o.lambda0, w.table, out.x ? out.x + m0 * F : w.A, w.t, w.lam, w.na, w.cfg, w.cfg_free);
      },
      [&](const RefineWs& w, int64_t m0, int mc, int) {
        const PosteriorOut oc = {rows_at(out.y, m0, nb),    rows_at(out.jac, m0, (int64_t)nb * F), rows_at(out.cov, m0, F * F),
                                 rows_at(out.ak, m0, F * F), rows_at(out.std, m0, F),              rows_at(out.dfs, m0, 1),
                                 rows_at(out.cost, m0, 1),   rows_at(out.nband, m0, 1),            rows_at(out.status, m0, 1)};
        hipLaunchKernelGGL(W == 8 ? k_refine_posterior<8> : k_refine_posterior<4>, dim3((unsigned)((mc + W - 1) / W)), dim3(64), lds, st, (const double*)w.cols,
                           rows_at(r.obs, m0, nb), rows_at(r.weights, m0, nb, o.weights_per_obs), o.weights_per_obs ? 1 : 0,
                           (const double*)w.cfg, mc, F, nb, (const double*)w.t, oc, rows_at(o.prior_mean, m0, F, o.prior_per_obs),
                           rows_at(o.prior_weight, m0, F, o.prior_per_obs), o.prior_per_obs ? 1 : 0);
      });
}

// spart_refine_views: the view-major table of k_refine_views_init, then n_iter + 1 times the forward call and the joint step
// kernel; o.prior_* are per unknown
static int views_impl(const RefineRun& r, const RefineOut& out, hipStream_t st) {
  const spart_refine_opt& o = r.o;
  const int nb = r.ctx->nb, V = r.s.V, F = r.s.F, Fs = r.s.Fs, n = r.s.n, rows = refine_lds_rows(F + 1, n, 0), W = refine_group(rows);
  const int64_t U = (int64_t)V * nb;
  const size_t lds = refine_lds_bytes(rows, W);
  return refine_loop(
      r, o.n_iter + 1, st,
      [&](const RefineWs& w, int64_t m0, int mc) {
        hipLaunchKernelGGL(k_refine_views_init, dim3((unsigned)(((int64_t)mc * V + 255) / 256)), dim3(256), 0, st, r.cfg, r.M, m0, mc, V,
                           F, Fs, o.lambda0, w.table, out.x + m0 * n, w.t, w.lam, w.na, w.cfg, w.cfg_free);
      },
      [&](const RefineWs& w, int64_t m0, int mc, int it) {
        ViewsStep a;
        a.cols = w.cols;
        a.obs = r.obs + m0 * U;
        a.wts = rows_at(r.weights, m0, U, o.weights_per_obs);
        a.cfg = w.cfg;
        a.cfg_free = w.cfg_free;
        a.table = w.table;
        a.Mc = mc, a.V = V, a.F = F, a.Fs = Fs, a.nb = nb, a.it = it, a.last = it == o.n_iter ? 1 : 0;
        a.wper = o.weights_per_obs ? 1 : 0, a.pper = o.prior_per_obs ? 1 : 0;
        a.st = w.t, a.sA = w.A, a.slam = w.lam, a.sna = w.na;
        a.out = rows_at(out, m0, r.s, nb);
        a.pmu = rows_at(o.prior_mean, m0, n, o.prior_per_obs);
        a.ppw = rows_at(o.prior_weight, m0, n, o.prior_per_obs);
        hipLaunchKernelGGL(W == 8 ? k_refine_views_step<8> : k_refine_views_step<4>, dim3((unsigned)((mc + W - 1) / W)), dim3(64), lds,
                           st, a);
      });
}

// spart_refine_mix: views' table in views' row order from k_refine_mix_init, then n_iter + 1 times the forward call and the
// mixture's step kernel; o.prior_* are per unknown, the fractions included
static int mix_impl(const RefineRun& r, const MixMap& map, int fit, double frac_lo, double frac_hi, const double* frac,
                    const MixOut& out, hipStream_t st) {
  const spart_refine_opt& o = r.o;
  const int nb = r.ctx->nb, V = r.s.V, F = r.s.F, Fs = r.s.Fs, n = r.s.n, rows = refine_lds_rows(n, n, MIX_MAXV), W = refine_group(rows);
  const size_t lds = refine_lds_bytes(rows, W);
  return refine_loop(
      r, o.n_iter + 1, st,
      [&](const RefineWs& w, int64_t m0, int mc) {
        MixInit a;
        a.cfg = r.cfg, a.map = map;
        a.M = r.M, a.m0 = m0, a.Mc = mc, a.V = V, a.F = F, a.Fs = Fs, a.fit = fit;
        a.lambda0 = o.lambda0, a.frac_lo = frac_lo, a.frac_hi = frac_hi;
        a.frac = frac;
        a.table = w.table, a.x = out.x + m0 * n, a.t = w.t, a.lam = w.lam, a.na = w.na, a.dcfg = w.cfg, a.dcfg_free = w.cfg_free;
        hipLaunchKernelGGL(k_refine_mix_init, dim3((unsigned)(((int64_t)mc * V + 255) / 256)), dim3(256), 0, st, a);
      },
      [&](const RefineWs& w, int64_t m0, int mc, int it) {
        MixStep a;
        a.cols = w.cols;
        a.obs = r.obs + m0 * nb;
        a.wts = rows_at(r.weights, m0, nb, o.weights_per_obs);
        a.cfg = w.cfg;
        a.frac = frac + m0 * V;
        a.cfg_free = w.cfg_free;
        a.table = w.table;
        a.Mc = mc, a.V = V, a.F = F, a.Fs = Fs, a.nb = nb, a.it = it, a.last = it == o.n_iter ? 1 : 0;
        a.wper = o.weights_per_obs ? 1 : 0, a.pper = o.prior_per_obs ? 1 : 0, a.fit = fit;
        a.st = w.t, a.sA = w.A, a.slam = w.lam, a.sna = w.na;
        a.out = {rows_at(out.x, m0, n),        rows_at(out.cost, m0, 1), rows_at(out.cost0, m0, 1), rows_at(out.sdev, m0, n),
                 rows_at(out.n_accept, m0, 1), rows_at(out.y, m0, nb),   rows_at(out.frac, m0, V),  rows_at(out.y_comp, m0, (int64_t)V * nb)};
        a.pmu = rows_at(o.prior_mean, m0, n, o.prior_per_obs);
        a.ppw = rows_at(o.prior_weight, m0, n, o.prior_per_obs);
        a.map = map;
        hipLaunchKernelGGL(W == 8 ? k_refine_mix_step<8> : k_refine_mix_step<4>, dim3((unsigned)((mc + W - 1) / W)), dim3(64), lds, st,
                           a);
      });
}

// What every entry point checks about the fit itself, in one order: the options (with the defaults that 0 stands for filled
// in), then every free column with its bounds, which become `cfg`.
static int refine_check_fit(const char* who, spart_refine_opt& o, int F, const int32_t* free_cols, const double* lo,
                            const double* hi, RefineCfg& cfg) {
  if (o.column < 0 || o.column > 2) return fail(SPART_ERR_INVALID, "%s: column = %d (0 R_TOC, 1 R_TOA, 2 L_TOA)", who, o.column);
  if (o.n_iter < 0 || o.n_iter > REFINE_MAX_ITER)
    return fail(SPART_ERR_INVALID, "%s: n_iter = %d, expected 0 ... %d", who, o.n_iter, REFINE_MAX_ITER);
  if (o.nlayers < 0 || o.nlayers > SPART_MAX_NLAYERS)
    return fail(SPART_ERR_INVALID, "%s: nlayers = %d (0 = the default 60, else 1 ... %d)", who, o.nlayers, SPART_MAX_NLAYERS);
  if (!(o.rel_step >= 0.0) || !(o.lambda0 >= 0.0) || std::isinf(o.rel_step) || std::isinf(o.lambda0))
    return fail(SPART_ERR_INVALID, "%s: rel_step and lambda0 must be finite and >= 0 (0 = the default)", who);
  if (o.prior_per_obs != 0 && o.prior_per_obs != 1)
    return fail(SPART_ERR_INVALID, "%s: prior_per_obs = %d (0: one row for all, 1: one row per observation)", who, o.prior_per_obs);
  if (!o.prior_mean != !o.prior_weight)
    return fail(SPART_ERR_INVALID, "%s: prior_mean and prior_weight come together (both NULL = no prior)", who);
  if (o.rel_step == 0.0) o.rel_step = 1e-3;
  if (o.lambda0 == 0.0) o.lambda0 = 1e-2;
  std::memset(&cfg, 0, sizeof(cfg));
  for (int f = 0; f < F; ++f) {
    const int c = free_cols[f];
    if (c < 0 || c >= SPART_NPARAM) return fail(SPART_ERR_INVALID, "%s: free_cols[%d] = %d, expected 0 ... %d", who, f, c, SPART_NPARAM - 1);
    if (cfg.is_free[c]) return fail(SPART_ERR_INVALID, "%s: column %d is free twice", who, c);
    if (!std::isfinite(lo[f]) || !std::isfinite(hi[f]) || !(lo[f] < hi[f]))
      return fail(SPART_ERR_INVALID, "%s: bounds of free_cols[%d]: finite lo < hi expected", who, f);
    cfg.is_free[c] = 1;
    cfg.free_col[f] = c;
    cfg.lo[f] = lo[f];
    cfg.hi[f] = hi[f];
    cfg.h[f] = o.rel_step * (hi[f] - lo[f]);
  }
  return SPART_OK;
}

static int refine_check_band_model(const char* who, int band_model) {
  if (band_model == 0 || band_model == 1) return SPART_OK;
  return fail(SPART_ERR_INVALID, "%s: band_model = %d (0 centre columns, 1 SRF columns)", who, band_model);
}

// What spart_sobol and spart_sample check first, and what they require of the caller's arrays with M > 0 ahead of their own
static int fit_check_head(const char* who, const spart_ctx* ctx, int F, const int32_t* free_cols, const double* lo, const double* hi) {
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (F < 1 || F > REFINE_MAXF) return fail(SPART_ERR_INVALID, "%s: F = %d, expected 1 <= F <= %d", who, F, REFINE_MAXF);
  if (!free_cols || !lo || !hi) return fail(SPART_ERR_INVALID, "%s: null argument (free_cols, lo and hi are required)", who);
  return SPART_OK;
}
static int fit_check_given(const char* who, const void* opt, const void* out, const double* const* base) {
  if (!opt) return fail(SPART_ERR_INVALID, "%s: opt is null", who);
  if (!out) return fail(SPART_ERR_INVALID, "%s: out is null", who);
  if (!base) return fail(SPART_ERR_INVALID, "%s: base is null", who);
  if (int i = first_null(base, SPART_NPARAM); i < SPART_NPARAM) return fail(SPART_ERR_INVALID, "%s: base[%d] is null", who, i);
  return SPART_OK;
}
// the kernel argument of either (SobolCfg, SampleCfg) from the checked fit
template <typename Cfg> static Cfg fit_cfg(const RefineCfg& rc, const double* const* base, int F) {
  Cfg c;
  std::memset(&c, 0, sizeof(c));
  for (int p = 0; p < SPART_NPARAM; ++p) c.base[p] = base[p], c.is_free[p] = rc.is_free[p];
  for (int f = 0; f < F; ++f) c.free_col[f] = rc.free_col[f], c.lo[f] = rc.lo[f], c.hi[f] = rc.hi[f];
  return c;
}

// the arguments the four entry points share
struct RefineArgs {
  spart_ctx* ctx;
  int64_t M;
  const double* const* base;
  int F;
  const int32_t* free_cols;
  const double *lo, *hi, *obs, *weights;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};

// The tail of every entry of the family, Sobol' and the sampler included, once its arguments are checked: the sensor, the
// empty call, then -- size(total) sizes the workspace and may still refuse what only a call with M > 0 needs -- the
// workspace's own check and the guarded call of run(st).
template <typename Size, typename Run>
static int fit_tail(const char* who, spart_ctx* ctx, int64_t M, void* workspace, size_t workspace_bytes, void* stream, Size&& size,
                    Run&& run) {
  if (ctx->nb == 0) return fail(SPART_ERR_NOSENSOR, "%s: context has no sensor", who);
  if (M == 0) return SPART_OK;
  size_t total = 0;
  if (int rc = size(total)) return rc;
  if (!workspace || workspace_bytes < total)
    return fail(SPART_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, total, workspace_bytes);
  return guarded(ctx, who, workspace, total, stream, run);
}

// The one argument check and refusal order of the family.  `have_opt`: the entry's own option and output structs are there;
// `have_data`: so are the obs, x and cost it requires.  before(r) reads the options into r.o, r.s and r.srf once they are
// known to be there and may refuse; after() may refuse once the fit is checked; run(r, st) queues the checked call.
// layout(r, total) lays the workspace out, gives its size and may refuse what the size depends on: the last check before the
// workspace's own.
template <typename Before, typename After, typename Layout, typename Run>
static int refine_entry_sized(const char* who, const RefineArgs& a, bool have_opt, bool have_data, Before&& before, After&& after,
                              Layout&& layout, Run&& run) {
  if (!a.ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (a.M < 0 || a.M > 2000000000LL) return fail(SPART_ERR_INVALID, "%s: M = %lld, expected 0 <= M <= 2e9", who, (long long)a.M);
  if (a.F < 1 || a.F > REFINE_MAXF) return fail(SPART_ERR_INVALID, "%s: F = %d, expected 1 <= F <= %d", who, a.F, REFINE_MAXF);
  if (!a.base || !a.free_cols || !a.lo || !a.hi || !have_opt) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  RefineRun r;
  r.ctx = a.ctx, r.M = a.M, r.obs = a.obs, r.weights = a.weights, r.wsp = (char*)a.workspace;
  r.s = {1, a.F, a.F, a.F};
  if (int rc = before(r)) return rc;
  if (int rc = refine_check_fit(who, r.o, a.F, a.free_cols, a.lo, a.hi, r.cfg)) return rc;
  if (int rc = after()) return rc;
  return fit_tail(
      who, a.ctx, a.M, a.workspace, a.workspace_bytes, a.stream,
      [&](size_t& total) {
        if (int i = first_null(a.base, SPART_NPARAM); i < SPART_NPARAM) return fail(SPART_ERR_INVALID, "%s: base[%d] is null", who, i);
        if (!have_data) return fail(SPART_ERR_INVALID, "%s: null argument (obs, x and cost are required)", who);
        if (r.o.weights_per_obs && !a.weights) return fail(SPART_ERR_INVALID, "%s: weights_per_obs without weights", who);
        for (int p = 0; p < SPART_NPARAM; ++p) r.cfg.base[p] = a.base[p];
        for (int f = 0; f < a.F; ++f) r.cfg.freebase[f] = a.base[r.cfg.free_col[f]];
        return layout(r, total);
      },
      [&](hipStream_t st) { return run(r, st); });
}
template <typename Before, typename After, typename Run>
static int refine_entry(const char* who, const RefineArgs& a, bool have_opt, bool have_data, Before&& before, After&& after, Run&& run) {
  return refine_entry_sized(
      who, a, have_opt, have_data, before, after, [&](RefineRun& r, size_t& total) {
        r.l = refine_layout(a.ctx->nb, a.M, r.s.V, r.s.F, r.s.n);
        total = r.l.total;
        return SPART_OK;
      },
      run);
}
static int refine_no_check() { return SPART_OK; }

static int refine_call(const char* who, bool srf, const RefineArgs& a, const spart_refine_opt* opt, const RefineOut& out) {
  return refine_entry(
      who, a, opt, a.obs && out.x && out.cost,
      [&](RefineRun& r) {
        r.o = *opt, r.srf = srf;
        return SPART_OK;
      },
      refine_no_check, [&](const RefineRun& r, hipStream_t st) { return refine_impl(r, out, st); });
}

// ---- spart_refine_tiles (csrc/spart_refine_tiles.h).  The forward block and the forward call are the family's; the state
// per pixel and per tile is its own.  A chunk is a run of whole tiles of at most mcap = min(M, tiles_chunk(F)) pixels, so its
// row count depends on the partition: the forward call's scratch is sized by carve_bound_f64, which holds for every row
// count up to the cap.
struct TilesLayout {
  int64_t mcap;                 // pixels per chunk
  ForwardBlock b;
  size_t cfg, cfg_free, lt, ct, Ap, Lp, zt, St, Lt, lam, live, na, code, flag, tstart, ptile, total;
};
static TilesLayout tiles_layout(int nb, int64_t M, int F, int Fs) {
  TilesLayout x;
  x.mcap = std::min<int64_t>(M, tiles_chunk(F));
  const size_t mc = (size_t)x.mcap, rows = mc * (size_t)(F + 1), P = (size_t)(refine_ntri(F) + F), Ps = (size_t)(refine_ntri(Fs) + Fs);
  const size_t Fl = (size_t)(F - Fs);
  Carver c;
  x.b = forward_block(c, nb, rows, carve_bound_f64((int64_t)rows));
  x.cfg = c.take(REFINE_CFG_DOUBLES * 8);
  x.cfg_free = c.take(REFINE_MAXF * 4);
  x.lt = c.take(mc * Fl * 8);
  x.ct = c.take(mc * 8);
  x.Ap = c.take(mc * P * 8);
  x.Lp = c.take(mc * P * 8);
  x.zt = c.take(mc * (size_t)Fs * 8);                               // (a chunk of mc pixels holds at most mc tiles)
  x.St = c.take(mc * Ps * 8);
  x.Lt = c.take(mc * Ps * 8);
  x.lam = c.take(mc * 8);
  x.live = c.take(mc * 4);
  x.na = c.take(mc * 4);
  x.code = c.take(mc * 4);
  x.flag = c.take(mc * 4);
  x.tstart = c.take((mc + 1) * 4);
  x.ptile = c.take(mc * 4);
  x.total = c.o;
  return x;
}

static bool tiles_sizes_ok(const spart_ctx* ctx, int64_t M, int F, int n_shared) {
  return fit_sizes_ok(ctx, M, F) && n_shared >= 0 && n_shared <= F;
}

// A chunk of tc whole groups (tiles, or series) from group t0, mc pixels from pixel m0, as the kernels of an iteration see it
struct TilesChunk {
  int64_t t0, m0;
  int tc, mc;
  unsigned per_pixel;           // blocks of 256 threads, one thread per pixel
  TilesState s;
  TilesOut oc;
  const double *ycol, *obs, *wts, *pmu, *ppw, *smu, *spw;
  int wper, pper, sper;
  double *table, *cfg;
  int32_t* cfg_free;
};

// The chunk loop over whole groups of the partition (T, start), for the tiles and the series: the group map of a chunk is
// built here, copied, and the stream waited for before the host copy goes away; then k_tiles_init and n_iter + 1 times the
// forward call and steps(chunk, it, last), the kernels of the entry.
template <typename Steps>
static int tiles_loop(const RefineRun& r, const TilesLayout& x, int64_t T, const int64_t* start, const spart_refine_tiles_opt& to,
                      const spart_tiles_out& out, hipStream_t st, Steps&& steps) {
  const spart_refine_opt& o = r.o;
  const int nb = r.ctx->nb, F = r.s.F, Fs = to.n_shared, Fl = F - Fs;
  const Forward fwd = r.forward(x.b);
  auto at = [&](size_t off) { return r.wsp + off; };
  TilesChunk c;
  c.s = {(double*)at(x.lt),   (double*)at(x.ct),   (double*)at(x.Ap),    (double*)at(x.Lp),    (double*)at(x.zt),
         (double*)at(x.St),   (double*)at(x.Lt),   (double*)at(x.lam),   (int32_t*)at(x.live), (int32_t*)at(x.na),
         (int32_t*)at(x.code), (int32_t*)at(x.flag), (int32_t*)at(x.tstart), (int32_t*)at(x.ptile)};
  c.ycol = fwd.y, c.table = fwd.table, c.cfg = (double*)at(x.cfg), c.cfg_free = (int32_t*)at(x.cfg_free);
  c.wper = o.weights_per_obs ? 1 : 0, c.pper = o.prior_per_obs ? 1 : 0, c.sper = to.shared_prior_per_tile ? 1 : 0;
  std::vector<int32_t> tstart, ptile;
  for (int64_t t0 = 0; t0 < T;) {
    const int64_t m0 = start[t0];
    int64_t t1 = t0 + 1;                                            // (one group always fits: TILES_MAXG, SERIES_MAXT <= tiles_chunk(16))
    while (t1 < T && start[t1 + 1] - m0 <= x.mcap) ++t1;
    const int tc = (int)(t1 - t0), mc = (int)(start[t1] - m0);
    tstart.resize((size_t)tc + 1);
    ptile.resize((size_t)mc);
    for (int t = 0; t <= tc; ++t) tstart[t] = (int32_t)(start[t0 + t] - m0);
    for (int t = 0; t < tc; ++t)
      for (int m = tstart[t]; m < tstart[t + 1]; ++m) ptile[m] = t;
    HIP_TRY(hipMemcpyAsync(c.s.tstart, tstart.data(), ((size_t)tc + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.s.ptile, ptile.data(), (size_t)mc * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.t0 = t0, c.m0 = m0, c.tc = tc, c.mc = mc, c.per_pixel = (unsigned)((mc + 255) / 256);
    c.oc = {rows_at(out.shared, t0, Fs),    rows_at(out.shared_std, t0, Fs), rows_at(out.local, m0, Fl),
            rows_at(out.local_std, m0, Fl), rows_at(out.cost, t0, 1),       rows_at(out.cost0, t0, 1),
            rows_at(out.n_accept, t0, 1),   rows_at(out.pixel_cost, m0, 1), rows_at(out.status, m0, 1),
            rows_at(out.y, m0, nb)};
    c.obs = r.obs + m0 * nb;
    c.wts = rows_at(r.weights, m0, nb, o.weights_per_obs);
    c.pmu = rows_at(o.prior_mean, m0, Fl, o.prior_per_obs);
    c.ppw = rows_at(o.prior_weight, m0, Fl, o.prior_per_obs);
    c.smu = rows_at(to.shared_prior_mean, t0, Fs, to.shared_prior_per_tile);
    c.spw = rows_at(to.shared_prior_weight, t0, Fs, to.shared_prior_per_tile);
    hipLaunchKernelGGL(k_tiles_init, dim3(c.per_pixel), dim3(256), 0, st, r.cfg, m0, mc, F, Fs, o.lambda0, c.s, c.table, c.oc, c.cfg,
                       c.cfg_free);
    HIP_TRY(hipGetLastError());
    const int64_t rows = (int64_t)mc * (F + 1);
    for (int it = 0; it <= o.n_iter; ++it) {
      if (int rc = fwd.run(rows, st)) return rc;
      steps(c, it, it == o.n_iter ? 1 : 0);
      HIP_TRY(hipGetLastError());
    }
    t0 = t1;
  }
  return SPART_OK;
}

// spart_refine_tiles: per iteration the six kernels, or seven with shared unknowns
static int tiles_impl(const RefineRun& r, const TilesLayout& x, int64_t T, const int64_t* tile_start, const spart_refine_tiles_opt& to,
                      const spart_tiles_out& out, hipStream_t st) {
  const int nb = r.ctx->nb, F = r.s.F, Fs = to.n_shared, Fl = F - Fs, P = refine_ntri(F) + F;
  const size_t lds = tiles_lds_bytes(F);
  return tiles_loop(r, x, T, tile_start, to, out, st, [&](const TilesChunk& c, int it, int last) {
    const int mc = c.mc, tc = c.tc;
    const unsigned groups = (unsigned)((mc + TILES_GROUP - 1) / TILES_GROUP);
    hipLaunchKernelGGL(k_tiles_cost, dim3(c.per_pixel), dim3(256), 0, st, c.ycol, c.obs, c.wts, c.wper, c.pmu, c.ppw, c.pper, mc, Fl, nb,
                       it, c.s, c.oc);
    hipLaunchKernelGGL(k_tiles_decide, dim3((unsigned)tc), dim3(64), 0, st, c.smu, c.spw, c.sper, Fs, it, last, c.s, c.oc);
    hipLaunchKernelGGL(k_tiles_normal, dim3((unsigned)(((int64_t)mc * P + 255) / 256)), dim3(256), 0, st, c.ycol, c.obs, c.wts, c.wper,
                       c.pmu, c.ppw, c.pper, (const double*)c.cfg, mc, F, Fs, nb, c.s, c.oc);
    hipLaunchKernelGGL(k_tiles_eliminate, dim3(groups), dim3(64), lds, st, mc, F, Fs, last, c.s);
    if (Fs > 0)                                                     // (without shared unknowns there is nothing to walk or to solve)
      hipLaunchKernelGGL(k_tiles_schur, dim3((unsigned)tc), dim3(TILES_SCHUR_THREADS), 0, st, c.smu, c.spw, c.sper, F, Fs, last, c.s, c.oc);
    hipLaunchKernelGGL(k_tiles_local, dim3(groups), dim3(64), lds, st, mc, F, Fs, last, c.s, c.oc);
    if (!last)
      hipLaunchKernelGGL(k_tiles_apply, dim3(c.per_pixel), dim3(256), 0, st, (const double*)c.cfg, (const int32_t*)c.cfg_free, c.table, mc,
                         F, Fs, c.s, c.oc);
  });
}

// ---- SRF support (include/spart_hip.h: spart_srf_support)
// The grid point of wlS (400..2400 by 1, 2500..15000 by 100, 16000..50000 by 1000) nearest to w in exact arithmetic: ties to
// the lower index, NaN -> 0.  With g[i] <= w <= g[i + 1] <= 2 g[i] both differences below are exact (Sterbenz), so the
// comparison is the exact one.
static int srf_grid_index(double w) {
  static const std::vector<double> g = [] {
    std::vector<double> v;
    for (int i = 0; i < NWL; ++i) v.push_back(400.0 + i);
    for (int i = 0; i <= 125; ++i) v.push_back(2500.0 + 100.0 * i);
    for (int i = 0; i <= 34; ++i) v.push_back(16000.0 + 1000.0 * i);
    return v;
  }();
  static_assert(NWL + 126 + 35 == NWLS, "the model grid");
  if (!(w > g.front())) return 0;                       // (NaN included)
  if (w >= g.back()) return NWLS - 1;
  const int i = (int)(std::upper_bound(g.begin(), g.end(), w) - g.begin()) - 1;      // g[i] <= w < g[i + 1]
  return (g[i + 1] - w) < (w - g[i]) ? i + 1 : i;
}

// Bands to the waves of k_columns_srf: sorted by support size, longest first (ties: the lower band), in groups of COL_WAVES;
// deal[COL_WAVES g + w] = the band of wave w of group g, the last group padded with -1.
static std::vector<int> srf_deal(const std::vector<int>& start, int nb) {
  std::vector<int> deal(nb);
  for (int j = 0; j < nb; ++j) deal[j] = j;
  std::stable_sort(deal.begin(), deal.end(), [&](int a, int b) { return start[a + 1] - start[a] > start[b + 1] - start[b]; });
  deal.resize((size_t)(nb + COL_WAVES - 1) / COL_WAVES * COL_WAVES, -1);
  return deal;
}

#ifndef SPART_BUILD_ID
#define SPART_BUILD_ID "unidentified"     // built outside spart-python_amd/build.py
#endif
// tag + id: build.py finds the id in the file's bytes (binary_id), spart_build_id() returns the part after the tag
static const char k_build_id[] = "SPART_BUILD_ID:" SPART_BUILD_ID;

// ---- spart_refine_leaf (csrc/spart_refine_leaf.h): one launch, no workspace
template <int F> static void launch_refine_leaf(int F_, unsigned blocks, hipStream_t st, const double* tab, const LeafFitArgs& a, int64_t M) {
  if constexpr (F <= LEAF_MAXF) {
    if (F_ == F) hipLaunchKernelGGL((k_refine_leaf<F>), dim3(blocks), dim3(LEAF_LANES), 0, st, tab, a, M);
    else launch_refine_leaf<F + 1>(F_, blocks, st, tab, a, M);
  }
}

extern "C" {

const char* spart_build_id(void) { return k_build_id + 15; }

int spart_abi_version(void) { return SPART_ABI_VERSION; }

const char* spart_last_error(const spart_ctx*) { return g_err; }

int spart_ctx_nb(const spart_ctx* ctx) { return ctx ? ctx->nb : 0; }

int spart_ctx_set_row_pitch(spart_ctx* ctx, int64_t pitch_full, int64_t pitch_optical) {
  if (!ctx) return fail(SPART_ERR_INVALID, "spart_ctx_set_row_pitch: null context");
  if (pitch_full == 0) pitch_full = NWLS;
  if (pitch_optical == 0) pitch_optical = NWL;
  if (pitch_full < NWLS || pitch_optical < NWL || pitch_full > (1 << 20) || pitch_optical > (1 << 20))
    return fail(SPART_ERR_INVALID, "row pitch must be >= the row width (%d / %d elements)", NWLS, NWL);
  std::lock_guard<std::mutex> lock(ctx->mu);
  ctx->pf = (int)pitch_full;
  ctx->po = (int)pitch_optical;
  return SPART_OK;
}

int spart_ctx_econv(const spart_ctx* ctx, double* host_out) {
  if (!ctx || !host_out) return fail(SPART_ERR_INVALID, "spart_ctx_econv: null argument");
  if (ctx->nb == 0) return fail(SPART_ERR_NOSENSOR, "context has no sensor");
  std::memcpy(host_out, ctx->econv_host.data(), sizeof(double) * ctx->nb);
  return SPART_OK;
}

int spart_ctx_destroy(spart_ctx* ctx) {
  if (!ctx) return SPART_OK;
  DeviceGuard g(ctx->device);
  (void)hipFree(ctx->tabF); (void)hipFree(ctx->tabD); (void)hipFree(ctx->Ea);
  (void)hipFree(ctx->band0); (void)hipFree(ctx->band1); (void)hipFree(ctx->frac); (void)hipFree(ctx->coef);
  (void)hipFree(ctx->econv);
  (void)hipFree(ctx->srf_start); (void)hipFree(ctx->srf_ev); (void)hipFree(ctx->srf_q); (void)hipFree(ctx->srf_Q);
  (void)hipFree(ctx->srf_deal);
  for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
  for (SideLane& l : ctx->lanes) {
    (void)hipEventDestroy(l.fork);
    (void)hipEventDestroy(l.join);
    (void)hipStreamDestroy(l.side);
  }
  for (WsUse& u : ctx->ws_uses) (void)hipEventDestroy(u.done);
  delete ctx;
  return SPART_OK;
}

int spart_ctx_create(spart_ctx** out, int device, const spart_tables* t) {
  if (!out || !t) return fail(SPART_ERR_INVALID, "spart_ctx_create: null argument");
  *out = nullptr;
  const double* req[] = {t->nr, t->Kab, t->Kca, t->Kdm, t->Kw, t->Ks, t->Kant, t->cbc, t->prot, t->GSV, t->nw, t->Ea};
  for (const double* p : req)
    if (!p) return fail(SPART_ERR_INVALID, "spart_ctx_create: a spectral table pointer is null");
  if (t->nb < 0 || t->nb > MAX_NB) return fail(SPART_ERR_INVALID, "spart_ctx_create: nb=%d out of range", t->nb);
  if (t->nb > 0 && (!t->wl_smac || !t->coef || !t->wl_srf || !t->p_srf || t->nsrf <= 0))
    return fail(SPART_ERR_INVALID, "spart_ctx_create: sensor block incomplete");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(SPART_ERR_HIP, "spart_ctx_create: no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(SPART_ERR_INVALID, "spart_ctx_create: device %d of %d", device, ndev);
  DeviceGuard guard(device);
  if (!guard.ok) return fail(SPART_ERR_HIP, "spart_ctx_create: cannot select device %d", device);

  struct Owner {         // the half-built context and the temporary SRF buffers, released on every return
    spart_ctx* ctx = new spart_ctx();
    double *d_w = nullptr, *d_p = nullptr;
    ~Owner() { (void)hipFree(d_w); (void)hipFree(d_p); spart_ctx_destroy(ctx); }
  } own;
  spart_ctx* ctx = own.ctx;
  ctx->device = device;
  // --- derived per-band tables, float64 on the host
  std::vector<double> tab((size_t)NTAB * NWL);
  const double tav90_2 = calculate_tav(90, 2.0);
  for (int i = 0; i < NWL; ++i) {
    tab[TAB_KAB * NWL + i] = t->Kab[i];
    tab[TAB_KCA * NWL + i] = t->Kca[i];
    tab[TAB_KDM * NWL + i] = t->Kdm[i];
    tab[TAB_KW * NWL + i] = t->Kw[i];
    tab[TAB_KS * NWL + i] = t->Ks[i];
    tab[TAB_KANT * NWL + i] = t->Kant[i];
    tab[TAB_CBC * NWL + i] = t->cbc[i];
    tab[TAB_PROT * NWL + i] = t->prot[i];
    double nr = t->nr[i], nw = t->nw[i];
    double t12 = calculate_tav(90, nr);                         // prospect_5d.py:202
    tab[TAB_TALF * NWL + i] = calculate_tav(40, nr);            // :200
    tab[TAB_T12 * NWL + i] = t12;
    tab[TAB_T21 * NWL + i] = t12 / (nr * nr);                   // :204
    tab[TAB_GSV0 * NWL + i] = t->GSV[3 * i + 0];
    tab[TAB_GSV1 * NWL + i] = t->GSV[3 * i + 1];
    tab[TAB_GSV2 * NWL + i] = t->GSV[3 * i + 2];
    tab[TAB_CBAC * NWL + i] = calculate_tav(90, 2.0 / nw) / tav90_2;   // bsm.py:111
    tab[TAB_PW * NWL + i] = 1.0 - calculate_tav(90, nw) / (nw * nw);   // bsm.py:115
    tab[TAB_RW * NWL + i] = 1.0 - calculate_tav(40, nw);               // bsm.py:119
  }
  std::vector<float> tabf(tab.begin(), tab.end());
  int rc;
  std::vector<double> ea(t->Ea, t->Ea + NWL);
  if ((rc = upload(&ctx->tabD, tab)) || (rc = upload(&ctx->tabF, tabf)) || (rc = upload(&ctx->Ea, ea))) return rc;
  for (int i = 0; i < NWL; ++i) {                   // the two denominators of spart_products
    ctx->ea_all = ctx->ea_all + ea[i];
    if (i == PRODUCTS_PAR_LAST) ctx->ea_par = ctx->ea_all;
  }

  // --- sensor block
  ctx->nb = t->nb;
  if (t->nb > 0) {
    std::vector<int> e0(t->nb), e1(t->nb);
    std::vector<double> fr(t->nb);
    for (int j = 0; j < t->nb; ++j) interp_support(t->wl_smac[j], e0[j], e1[j], fr[j]);
    std::vector<double> coef(t->coef, t->coef + (size_t)NCOEF * t->nb);
    std::vector<double> wsrf(t->wl_srf, t->wl_srf + (size_t)t->nsrf * t->nb), psrf(t->p_srf, t->p_srf + (size_t)t->nsrf * t->nb);
    std::vector<double> ec(t->nb, 0.0);
    if ((rc = upload(&ctx->band0, e0)) || (rc = upload(&ctx->band1, e1)) || (rc = upload(&ctx->frac, fr)) ||
        (rc = upload(&ctx->coef, coef)) || (rc = upload(&ctx->econv, ec)) || (rc = upload(&own.d_w, wsrf)) ||
        (rc = upload(&own.d_p, psrf)))
      return rc;
    // compressed SRF support of the bands, for k_columns_srf
    std::vector<int> sst(t->nb + 1);
    if ((rc = spart_srf_support(t->wl_srf, t->p_srf, t->nsrf, t->nb, sst.data(), nullptr, nullptr, nullptr))) return rc;
    std::vector<int> sev(sst[t->nb]);
    std::vector<double> sq(sst[t->nb]), sQ(t->nb);
    if ((rc = spart_srf_support(t->wl_srf, t->p_srf, t->nsrf, t->nb, sst.data(), sev.data(), sq.data(), sQ.data()))) return rc;
    if ((rc = upload(&ctx->srf_start, sst)) || (rc = upload(&ctx->srf_ev, sev)) || (rc = upload(&ctx->srf_q, sq)) ||
        (rc = upload(&ctx->srf_Q, sQ)) || (rc = upload(&ctx->srf_deal, srf_deal(sst, t->nb))))
      return rc;
    // SRF convolution of the ET irradiance: one wave per sensor band (SPART.py:358-396)
    hipLaunchKernelGGL(k_econv, dim3(t->nb), dim3(64), 0, 0, ctx->Ea, own.d_w, own.d_p, t->nsrf, t->nb, ctx->econv);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    ctx->econv_host.resize(t->nb);
    if (e == hipSuccess) e = hipMemcpy(ctx->econv_host.data(), ctx->econv, sizeof(double) * t->nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SPART_ERR_HIP, "spart_ctx_create: SRF convolution kernel: %s", hipGetErrorString(e));
  }
  {
    const char* e = std::getenv("SPART_SIDE_STREAM");            // "0" keeps every kernel on the caller's stream
    ctx->side_enabled = !(e && e[0] == '0');
    ctx->lanes.reserve(MAX_LANES);                                // (pointers into the vector stay valid)
    ctx->ws_uses.reserve(WS_PRUNE_AT);
  }
  *out = ctx;
  own.ctx = nullptr;                                              // (the caller's now)
  return SPART_OK;
}

size_t spart_refine_workspace_bytes(const spart_ctx* ctx, int64_t M, int F) {
  return refine_sizes_ok(ctx, M, 1, F, F) ? refine_layout(ctx->nb, M, 1, F, F).total : 0;
}

size_t spart_views_workspace_bytes(const spart_ctx* ctx, int64_t M, int V, int F, int n_shared) {
  return refine_sizes_ok(ctx, M, V, F, n_shared) ? refine_layout(ctx->nb, M, V, F, n_shared + V * (F - n_shared)).total : 0;
}

int spart_refine(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols,
                 const double* lo, const double* hi, const double* obs, const double* weights, const spart_refine_opt* opt,
                 double* x, double* cost, double* cost0, double* sdev, int32_t* n_accept, double* y, void* workspace,
                 size_t workspace_bytes, void* stream) {
  return refine_call("spart_refine", false, {ctx, M, base, F, free_cols, lo, hi, obs, weights, workspace, workspace_bytes, stream}, opt,
                     {x, cost, cost0, sdev, n_accept, y});
}

int spart_refine_srf(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols,
                     const double* lo, const double* hi, const double* obs, const double* weights, const spart_refine_opt* opt,
                     double* x, double* cost, double* cost0, double* sdev, int32_t* n_accept, double* y, void* workspace,
                     size_t workspace_bytes, void* stream) {
  return refine_call("spart_refine_srf", true, {ctx, M, base, F, free_cols, lo, hi, obs, weights, workspace, workspace_bytes, stream},
                     opt, {x, cost, cost0, sdev, n_accept, y});
}

// obs may be NULL here, and the outputs come in one struct, of which one at least is asked for
int spart_refine_posterior(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols,
                           const double* lo, const double* hi, const double* obs, const double* weights,
                           const spart_refine_opt* opt, int band_model, const spart_posterior_out* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const char* who = "spart_refine_posterior";
  spart_posterior_out oo;
  return refine_entry(
      who, {ctx, M, base, F, free_cols, lo, hi, obs, weights, workspace, workspace_bytes, stream}, opt && out, true,
      [&](RefineRun& r) {
        r.o = *opt, r.srf = band_model == 1, oo = *out;
        return SPART_OK;
      },
      [&] {
        if (int rc = refine_check_band_model(who, band_model)) return rc;
        if (!oo.x && !oo.y && !oo.jac && !oo.cov && !oo.ak && !oo.std && !oo.dfs && !oo.cost && !oo.nband && !oo.status)
          return fail(SPART_ERR_INVALID, "%s: every output is null", who);
        return SPART_OK;
      },
      [&](const RefineRun& r, hipStream_t st) { return posterior_impl(r, oo, st); });
}

// the sizes of the views are checked once the options they are read from are known to be there, before the fit
int spart_refine_views(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols,
                       const double* lo, const double* hi, const double* obs, const double* weights,
                       const spart_refine_views_opt* opt, double* x, double* cost, double* cost0, double* sdev, int32_t* n_accept,
                       double* y, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_refine_views";
  const RefineOut out = {x, cost, cost0, sdev, n_accept, y};
  return refine_entry(
      who, {ctx, M, base, F, free_cols, lo, hi, obs, weights, workspace, workspace_bytes, stream}, opt, obs && x && cost,
      [&](RefineRun& r) {
        const int V = opt->V, Fs = opt->n_shared;
        if (V < 1 || V > VIEWS_MAXV) return fail(SPART_ERR_INVALID, "%s: V = %d, expected 1 <= V <= %d", who, V, VIEWS_MAXV);
        if (Fs < 0 || Fs > F) return fail(SPART_ERR_INVALID, "%s: n_shared = %d, expected 0 ... F = %d", who, Fs, F);
        const int n = Fs + V * (F - Fs);
        if (n < 1 || n > REFINE_MAXF)
          return fail(SPART_ERR_INVALID, "%s: n_shared + V (F - n_shared) = %d unknowns per pixel, expected 1 ... %d", who, n, REFINE_MAXF);
        r.o = opt->fit, r.srf = opt->band_model == 1, r.s = {V, F, Fs, n};
        return refine_check_band_model(who, opt->band_model);
      },
      refine_no_check, [&](const RefineRun& r, hipStream_t st) { return views_impl(r, out, st); });
}

size_t spart_mix_workspace_bytes(const spart_ctx* ctx, int64_t M, int V, int F, int n) {
  if (!fit_sizes_ok(ctx, M, F) || V < 1 || V > MIX_MAXV || n < 1 || n > REFINE_MAXF) return 0;
  return refine_layout(ctx->nb, M, V, F, n).total;
}

// the mixture's own refusals come once the options they are read from are known to be there, before the fit, as for the views
int spart_refine_mix(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols,
                     const double* lo, const double* hi, const double* obs, const double* weights, const double* frac,
                     const spart_refine_mix_opt* opt, const spart_refine_mix_out* out, void* workspace, size_t workspace_bytes,
                     void* stream) {
  const char* who = "spart_refine_mix";
  MixMap map;
  MixOut oo;
  int fit = 0;
  double flo = 0.0, fhi = 1.0;
  return refine_entry(
      who, {ctx, M, base, F, free_cols, lo, hi, obs, weights, workspace, workspace_bytes, stream}, opt && out,
      obs && out && out->x && out->cost,
      [&](RefineRun& r) {
        const int V = opt->V, Fs = opt->n_shared;
        if (V < 1 || V > MIX_MAXV) return fail(SPART_ERR_INVALID, "%s: V = %d, expected 1 <= V <= %d", who, V, MIX_MAXV);
        if (Fs < 0 || Fs > F) return fail(SPART_ERR_INVALID, "%s: n_shared = %d, expected 0 ... F = %d", who, Fs, F);
        if (int rc = refine_check_band_model(who, opt->band_model)) return rc;
        if (opt->fit_fractions != 0 && opt->fit_fractions != 1)
          return fail(SPART_ERR_INVALID, "%s: fit_fractions = %d (0: given, 1: fitted on the simplex)", who, opt->fit_fractions);
        const int Fl = F - Fs;
        if (opt->local_active)
          for (int i = 0; i < V * Fl; ++i)
            if (opt->local_active[i] != 0 && opt->local_active[i] != 1)
              return fail(SPART_ERR_INVALID, "%s: local_active[%d] = %d, expected 0 / 1", who, i, opt->local_active[i]);
        fit = opt->fit_fractions;
        const int n = mix_build_map(V, Fs, Fl, opt->local_active, fit, &map);
        if (n == -1) return fail(SPART_ERR_INVALID, "%s: a local name is active in no component", who);
        if (n < 1 || n > REFINE_MAXF)
          return fail(SPART_ERR_INVALID, "%s: the unknowns per pixel (shared + active locals + fitted fractions): expected 1 ... %d", who,
                      REFINE_MAXF);
        if (opt->frac_lo != 0.0 || opt->frac_hi != 0.0) {
          flo = opt->frac_lo, fhi = opt->frac_hi;
          if (!(flo >= 0.0 && flo < fhi && fhi <= 1.0))
            return fail(SPART_ERR_INVALID, "%s: fraction box (%g, %g): both 0 = [0, 1], else 0 <= lo < hi <= 1", who, flo, fhi);
        }
        if (!frac) return fail(SPART_ERR_INVALID, "%s: frac is null", who);
        r.o = opt->fit, r.srf = opt->band_model == 1, r.s = {V, F, Fs, n};
        oo = {out->x, out->cost, out->cost0, out->std, out->n_accept, out->y, out->frac, out->y_comp};
        return SPART_OK;
      },
      refine_no_check, [&](const RefineRun& r, hipStream_t st) { return mix_impl(r, map, fit, flo, fhi, frac, oo, st); });
}

size_t spart_tiles_workspace_bytes(const spart_ctx* ctx, int64_t M, int F, int n_shared) {
  return tiles_sizes_ok(ctx, M, F, n_shared) ? tiles_layout(ctx->nb, M, F, n_shared).total : 0;
}

// What spart_refine_tiles and spart_refine_series check about the partition and the shared prior, in one order, after the
// family's list and before the workspace's size
static int tiles_check(const char* who, const spart_refine_tiles_opt& to, int64_t M, int F, int64_t T, const int64_t* tile_start,
                       const char* count, const char* name, const char* units, const char* per, int maxg) {
  if (to.n_shared < 0 || to.n_shared > F) return fail(SPART_ERR_INVALID, "%s: n_shared = %d, expected 0 ... F = %d", who, to.n_shared, F);
  if (int rc = refine_check_band_model(who, to.band_model)) return rc;
  if (T < 0 || (T == 0 && M > 0))
    return fail(SPART_ERR_INVALID, "%s: %s = %lld %s for M = %lld pixels", who, count, (long long)T, units, (long long)M);
  if (!tile_start) return fail(SPART_ERR_INVALID, "%s: %s is null", who, name);
  if (tile_start[0] != 0) return fail(SPART_ERR_INVALID, "%s: %s[0] = %lld, expected 0", who, name, (long long)tile_start[0]);
  for (int64_t t = 1; t <= T; ++t) {
    const int64_t g = tile_start[t] - tile_start[t - 1];
    if (g < 1 || g > maxg || tile_start[t] > M)
      return fail(SPART_ERR_INVALID, "%s: %s[%lld] = %lld after %lld: 1 ... %d %s within M = %lld expected", who, name, (long long)t,
                  (long long)tile_start[t], (long long)tile_start[t - 1], maxg, per, (long long)M);
  }
  if (tile_start[T] != M)
    return fail(SPART_ERR_INVALID, "%s: %s[%lld] = %lld, expected M = %lld", who, name, (long long)T, (long long)tile_start[T], (long long)M);
  if (!to.shared_prior_mean != !to.shared_prior_weight)
    return fail(SPART_ERR_INVALID, "%s: shared_prior_mean and shared_prior_weight come together (both NULL = no prior)", who);
  if (to.shared_prior_per_tile != 0 && to.shared_prior_per_tile != 1)
    return fail(SPART_ERR_INVALID, "%s: shared_prior_per_tile = %d (0: one row for all, 1: one row per tile)", who, to.shared_prior_per_tile);
  return SPART_OK;
}

// spart_refine's refusals in refine_entry's order; what is about the tiles comes after them and before the workspace's size,
// which n_shared decides
int spart_refine_tiles(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols,
                       const double* lo, const double* hi, int64_t T, const int64_t* tile_start, const double* obs,
                       const double* weights, const spart_refine_tiles_opt* opt, const spart_tiles_out* out, void* workspace,
                       size_t workspace_bytes, void* stream) {
  const char* who = "spart_refine_tiles";
  spart_refine_tiles_opt to;
  spart_tiles_out oo;
  TilesLayout x;
  const bool have_out = opt && out && out->cost && (out->shared || opt->n_shared <= 0) && (out->local || opt->n_shared >= F);
  return refine_entry_sized(
      who, {ctx, M, base, F, free_cols, lo, hi, obs, weights, workspace, workspace_bytes, stream}, opt && out, obs && have_out,
      [&](RefineRun& r) {
        to = *opt, oo = *out;
        r.o = to.fit, r.srf = to.band_model == 1;
        return SPART_OK;
      },
      refine_no_check,
      [&](RefineRun&, size_t& total) {
        if (int rc = tiles_check(who, to, M, F, T, tile_start, "T", "tile_start", "tiles", "pixels per tile", TILES_MAXG)) return rc;
        x = tiles_layout(ctx->nb, M, F, to.n_shared);
        total = x.total;
        return SPART_OK;
      },
      [&](const RefineRun& r, hipStream_t st) { return tiles_impl(r, x, T, tile_start, to, oo, st); });
}

// ---- spart_refine_series (csrc/spart_refine_series.h).  The layout is tiles' with the factors of the link blocks, Xp
// (mcap, Fl Fl), and gamma (REFINE_MAXF) behind it; the chunk loop is tiles_loop over whole series.
struct SeriesLayout {
  TilesLayout x;
  size_t Xp, gamma, total;
};
static SeriesLayout series_layout(int nb, int64_t M, int F, int Fs) {
  SeriesLayout y;
  y.x = tiles_layout(nb, M, F, Fs);
  const size_t Fl = (size_t)(F - Fs);
  Carver c;
  c.take(y.x.total);
  y.Xp = c.take((size_t)y.x.mcap * Fl * Fl * 8);
  y.gamma = c.take(REFINE_MAXF * 8);
  y.total = c.o;
  return y;
}

// gamma goes up once, ahead of the loop: so.smooth is the caller's host memory, and the first chunk's wait for the stream
// comes before this returns.  Per iteration tiles' cost and normal kernels around the series' own.
static int series_impl(const RefineRun& r, const SeriesLayout& y, int64_t T, const int64_t* series_start,
                       const spart_refine_series_opt& so, const spart_tiles_out& out, hipStream_t st) {
  const int nb = r.ctx->nb, F = r.s.F, Fs = so.tiles.n_shared, Fl = F - Fs, P = refine_ntri(F) + F, Ps = refine_ntri(Fs) + Fs;
  const int W = series_group(F);
  const size_t lds_f = series_factor_lds(F, Fs, W), lds_b = series_back_lds(F, Fs, W), lds_s = series_std_lds(F, Fs);
  double* Xp = (double*)(r.wsp + y.Xp);
  double* gamma = (double*)(r.wsp + y.gamma);
  const bool want_std = out.shared_std || out.local_std;
  HIP_TRY(hipMemcpyAsync(gamma, so.smooth, (size_t)Fl * 8, hipMemcpyHostToDevice, st));
  return tiles_loop(r, y.x, T, series_start, so.tiles, out, st, [&](const TilesChunk& c, int it, int last) {
    const int mc = c.mc, tc = c.tc;
    const unsigned groups = (unsigned)((tc + W - 1) / W);
    const double* link = rows_at(so.link, c.m0, 1);
    hipLaunchKernelGGL(k_tiles_cost, dim3(c.per_pixel), dim3(256), 0, st, c.ycol, c.obs, c.wts, c.wper, c.pmu, c.ppw, c.pper, mc, Fl, nb,
                       it, c.s, c.oc);
    hipLaunchKernelGGL(k_series_decide, dim3((unsigned)((tc + 255) / 256)), dim3(256), 0, st, c.smu, c.spw, c.sper, tc, Fs, Fl, it, last,
                       (const double*)gamma, link, c.s, c.oc);
    hipLaunchKernelGGL(k_tiles_normal, dim3((unsigned)(((int64_t)mc * P + 255) / 256)), dim3(256), 0, st, c.ycol, c.obs, c.wts, c.wper,
                       c.pmu, c.ppw, c.pper, (const double*)c.cfg, mc, F, Fs, nb, c.s, c.oc);
    if (!last || want_std) {                                        // (the sums of the last point are only for the std)
      hipLaunchKernelGGL(k_series_augment, dim3((unsigned)(((int64_t)mc * Fl + 255) / 256)), dim3(256), 0, st, mc, F, Fs,
                         (const double*)gamma, link, c.s);
      if (Fs > 0)
        hipLaunchKernelGGL(k_series_sums, dim3((unsigned)(((int64_t)tc * Ps + 255) / 256)), dim3(256), 0, st, c.smu, c.spw, c.sper, tc,
                           F, Fs, c.s, c.oc);
      hipLaunchKernelGGL(W == 8 ? k_series_factor<8> : k_series_factor<4>, dim3(groups), dim3(64), lds_f, st, tc, F, Fs, last,
                         (const double*)gamma, link, c.s, Xp);
      if (Fs > 0)
        hipLaunchKernelGGL(k_series_shared, dim3((unsigned)((tc + SERIES_STD_THREADS - 1) / SERIES_STD_THREADS)),
                           dim3(SERIES_STD_THREADS), (size_t)Fs * SERIES_STD_THREADS * 8, st, tc, Fs, last, c.s, c.oc.shared_std);
    }
    if (!last) {
      hipLaunchKernelGGL(W == 8 ? k_series_back<8> : k_series_back<4>, dim3(groups), dim3(64), lds_b, st, tc, F, Fs,
                         (const double*)gamma, link, c.s, (const double*)Xp);
      hipLaunchKernelGGL(k_tiles_apply, dim3(c.per_pixel), dim3(256), 0, st, (const double*)c.cfg, (const int32_t*)c.cfg_free, c.table, mc,
                         F, Fs, c.s, c.oc);
    } else if (out.local_std) {
      hipLaunchKernelGGL(k_series_std, dim3((unsigned)((mc + SERIES_STD_THREADS - 1) / SERIES_STD_THREADS)), dim3(SERIES_STD_THREADS),
                         lds_s, st, mc, F, Fs, (const double*)gamma, link, c.s, (const double*)Xp, c.oc.local_std);
    }
  });
}

size_t spart_series_workspace_bytes(const spart_ctx* ctx, int64_t M, int F, int n_shared) {
  return tiles_sizes_ok(ctx, M, F, n_shared) && n_shared < F ? series_layout(ctx->nb, M, F, n_shared).total : 0;
}

// spart_refine_tiles' refusals in its order (series_start under the 256-row rule), then Fl = 0, then smooth; the workspace last
int spart_refine_series(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols,
                        const double* lo, const double* hi, int64_t S, const int64_t* series_start, const double* obs,
                        const double* weights, const spart_refine_series_opt* opt, const spart_tiles_out* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const char* who = "spart_refine_series";
  spart_refine_series_opt so;
  spart_tiles_out oo;
  SeriesLayout y;
  const bool have_out =
      opt && out && out->cost && (out->shared || opt->tiles.n_shared <= 0) && (out->local || opt->tiles.n_shared >= F);
  return refine_entry_sized(
      who, {ctx, M, base, F, free_cols, lo, hi, obs, weights, workspace, workspace_bytes, stream}, opt && out, obs && have_out,
      [&](RefineRun& r) {
        so = *opt, oo = *out;
        r.o = so.tiles.fit, r.srf = so.tiles.band_model == 1;
        return SPART_OK;
      },
      refine_no_check,
      [&](RefineRun&, size_t& total) {
        if (int rc = tiles_check(who, so.tiles, M, F, S, series_start, "S", "series_start", "series", "rows per series", SERIES_MAXT))
          return rc;
        const int Fl = F - so.tiles.n_shared;
        if (Fl == 0) return fail(SPART_ERR_INVALID, "%s: n_shared = F = %d, nothing to link: use spart_refine_tiles", who, F);
        if (!so.smooth) return fail(SPART_ERR_INVALID, "%s: smooth is null", who);
        for (int b = 0; b < Fl; ++b)
          if (!(so.smooth[b] >= 0.0) || std::isinf(so.smooth[b]))
            return fail(SPART_ERR_INVALID, "%s: smooth[%d] = %g, expected a finite value >= 0", who, b, so.smooth[b]);
        y = series_layout(ctx->nb, M, F, so.tiles.n_shared);
        total = y.total;
        return SPART_OK;
      },
      [&](const RefineRun& r, hipStream_t st) { return series_impl(r, y, S, series_start, so, oo, st); });
}

// ---- spart_sobol (csrc/spart_sobol.h).  Workspace: ONE chunk of forward rows -- the forward block of R = 64 (F + 2) bcap
// rows -- then c_j and the block sums of the nslot sites a chunk can touch ((N / 64) nb Q doubles each).
// bcap = min(M G, sobol_chunk_blocks(F)) blocks, G = N / 64: it depends on M only while the whole call is smaller than one
// chunk.
struct SobolLayout {
  int64_t bcap;                 // blocks per chunk
  int nslot;                    // sites whose block sums are kept at once
  ForwardBlock b;
  size_t cbuf, bs, total;
};
static SobolLayout sobol_layout(int nb, int64_t M, int64_t N, int F) {
  SobolLayout l;
  const int64_t G = N / SOBOL_BLOCK;
  l.bcap = std::min<int64_t>(M * G, sobol_chunk_blocks(F));
  l.nslot = (int)std::min<int64_t>(M, l.bcap / G + 2);            // (bc consecutive blocks touch at most bc / G + 2 sites)
  const size_t rows = (size_t)l.bcap * SOBOL_BLOCK * (size_t)(F + 2);
  Carver c;
  l.b = forward_block(c, nb, rows, carve_bound_f64((int64_t)rows));
  l.cbuf = c.take((size_t)l.nslot * nb * 8);
  l.bs = c.take((size_t)l.nslot * (size_t)G * (size_t)sobol_nq(F) * nb * 8);
  l.total = c.o;
  return l;
}

static bool sobol_n_ok(int64_t N) { return N >= SOBOL_MIN_N && N <= SOBOL_MAX_N && N % SOBOL_BLOCK == 0; }

size_t spart_sobol_workspace_bytes(const spart_ctx* ctx, int64_t M, int64_t N, int F) {
  return fit_sizes_ok(ctx, M, F) && sobol_n_ok(N) ? sobol_layout(ctx->nb, M, N, F).total : 0;
}

// the chunk loop: the table, the forward call, the block sums, then the sites whose last block lies in the chunk
static int sobol_impl(spart_ctx* ctx, const SobolCfg& cfg, int64_t M, int F, int64_t N, const double* uA, const double* uB,
                      const spart_sobol_opt& o, const SobolOut& out, char* wsp, const SobolLayout& l, hipStream_t st) {
  const int nb = ctx->nb, G = (int)(N / SOBOL_BLOCK), per = SOBOL_BLOCK * (F + 2);
  const Forward fwd(ctx, wsp, l.b, o.column, o.band_model == 1, o.fast_prelude, o.nlayers);
  double* cbuf = (double*)(wsp + l.cbuf);
  double* bs = (double*)(wsp + l.bs);
  const int64_t B = M * G;
  for (int64_t b0 = 0; b0 < B; b0 += l.bcap) {
    const int bc = (int)std::min<int64_t>(l.bcap, B - b0);
    const int64_t rows = (int64_t)bc * per;
    hipLaunchKernelGGL(k_sobol_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, cfg, F, b0, bc, G, uA, uB, fwd.table);
    HIP_TRY(hipGetLastError());
    if (int rc = fwd.run(rows, st)) return rc;
    hipLaunchKernelGGL(k_sobol_blocks, dim3((unsigned)(((int64_t)bc * nb + 3) / 4)), dim3(256), 0, st, fwd.y, nb, F, b0, bc, G, l.nslot,
                       cbuf, bs);
    const int64_t m0 = b0 / G, m1 = (b0 + bc) / G;                 // sites m0 <= m < m1 end in this chunk
    if (m1 > m0)
      hipLaunchKernelGGL(k_sobol_finish, dim3((unsigned)((nb * F + 63) / 64), (unsigned)(m1 - m0)), dim3(64), 0, st,
                         (const double*)bs, (const double*)cbuf, nb, F, G, l.nslot, m0, (double)N, out);
    HIP_TRY(hipGetLastError());
  }
  return SPART_OK;
}

// spart_refine's checks of F, the four host arrays, the options and the free columns in its order (refine_check_fit on a
// zeroed spart_refine_opt that carries column and nlayers); then band_model, N, M; then, with M > 0, what is NULL; the
// workspace last
int spart_sobol(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols, const double* lo,
                const double* hi, int64_t N, const double* uA, const double* uB, const spart_sobol_opt* opt,
                const spart_sobol_out* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_sobol";
  if (int r = fit_check_head(who, ctx, F, free_cols, lo, hi)) return r;
  spart_sobol_opt o;
  std::memset(&o, 0, sizeof(o));
  if (opt) o = *opt;
  spart_refine_opt ro;
  std::memset(&ro, 0, sizeof(ro));
  ro.column = o.column, ro.nlayers = o.nlayers;
  RefineCfg rc;
  if (int r = refine_check_fit(who, ro, F, free_cols, lo, hi, rc)) return r;
  if (int r = refine_check_band_model(who, o.band_model)) return r;
  if (!sobol_n_ok(N))
    return fail(SPART_ERR_INVALID, "%s: N = %lld, expected a multiple of %d in %lld ... %lld", who, (long long)N, SOBOL_BLOCK,
                (long long)SOBOL_MIN_N, (long long)SOBOL_MAX_N);
  if (M < 0 || M > 2000000000LL) return fail(SPART_ERR_INVALID, "%s: M = %lld, expected 0 <= M <= 2e9", who, (long long)M);
  if (M > 0) {
    if (int r = fit_check_given(who, opt, out, base)) return r;
    if (!uA) return fail(SPART_ERR_INVALID, "%s: uA is null", who);
    if (!uB) return fail(SPART_ERR_INVALID, "%s: uB is null", who);
    if (!out->mean && !out->var && !out->S1 && !out->ST && !out->S1_se && !out->ST_se)
      return fail(SPART_ERR_INVALID, "%s: every output is null", who);
  }
  SobolLayout l;
  return fit_tail(
      who, ctx, M, workspace, workspace_bytes, stream,
      [&](size_t& total) {
        l = sobol_layout(ctx->nb, M, N, F);
        total = l.total;
        return SPART_OK;
      },
      [&](hipStream_t st) {
        const SobolCfg cfg = fit_cfg<SobolCfg>(rc, base, F);
        const SobolOut so = {out->mean, out->var, out->S1, out->ST, out->S1_se, out->ST_se};
        return sobol_impl(ctx, cfg, M, F, N, uA, uB, o, so, (char*)workspace, l, st);
      });
}

// ---- spart_vjp (csrc/spart_vjp.h).  Workspace: ONE chunk of Mc = min(M, vjp_chunk(F)) observations -- the forward block of
// 2 F Mc rows -- then the chunk's denominators a_f - b_f.  The call's constants travel as k_vjp_init's argument: no kernel
// after it reads them, so they have no device copy.
struct VjpLayout {
  int64_t mcap;                 // observations per chunk
  ForwardBlock b;
  size_t den, total;
};
static VjpLayout vjp_layout(int nb, int64_t M, int F) {
  VjpLayout l;
  l.mcap = std::min<int64_t>(M, vjp_chunk(F));
  const size_t rows = (size_t)l.mcap * 2 * (size_t)F;
  Carver c;
  l.b = forward_block(c, nb, rows, carve_bound_f64((int64_t)rows));
  l.den = c.take((size_t)l.mcap * F * 8);
  l.total = c.o;
  return l;
}

size_t spart_vjp_workspace_bytes(const spart_ctx* ctx, int64_t M, int F) {
  return fit_sizes_ok(ctx, M, F) ? vjp_layout(ctx->nb, M, F).total : 0;
}

// the chunk loop: the table, ONE forward call, the sums
static int vjp_impl(spart_ctx* ctx, const RefineCfg& cfg, int64_t M, int F, const double* const gy[3], int column,
                    const spart_vjp_opt& o, double* grad, char* wsp, const VjpLayout& l, hipStream_t st) {
  const int nb = ctx->nb, W = vjp_group_lds(F);
  const Forward fwd(ctx, wsp, l.b, column, o.band_model == 1, o.fast_prelude, o.nlayers);
  double* den = (double*)(wsp + l.den);
  for (int64_t m0 = 0; m0 < M; m0 += l.mcap) {
    const int mc = (int)std::min<int64_t>(l.mcap, M - m0);
    hipLaunchKernelGGL(k_vjp_init, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, st, cfg, m0, mc, F, fwd.table, den);
    HIP_TRY(hipGetLastError());
    if (int rc = fwd.run((int64_t)mc * 2 * F, st)) return rc;
    VjpCols a;
    for (int c = 0; c < 3; ++c) a.y[c] = fwd.cols[c], a.g[c] = rows_at(gy[c], m0, nb);
    hipLaunchKernelGGL(k_vjp_reduce, dim3((unsigned)((mc + W - 1) / W)), dim3(64), vjp_lds_bytes(F, W), st, a, (const double*)den, mc,
                       F, nb, W, grad + m0 * F);
    HIP_TRY(hipGetLastError());
  }
  return SPART_OK;
}

// spart_sobol's head (F, the host arrays, nlayers, the free columns and their bounds: refine_check_fit on a zeroed
// spart_refine_opt that carries nlayers); then opt, band_model, rel_step, gy, grad, M; then, with M > 0, base; the sensor and
// the workspace last
int spart_vjp(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols, const double* lo,
              const double* hi, const double* const gy[3], const spart_vjp_opt* opt, double* grad, void* workspace,
              size_t workspace_bytes, void* stream) {
  const char* who = "spart_vjp";
  if (int r = fit_check_head(who, ctx, F, free_cols, lo, hi)) return r;
  spart_vjp_opt o;
  std::memset(&o, 0, sizeof(o));
  if (opt) o = *opt;
  spart_refine_opt ro;
  std::memset(&ro, 0, sizeof(ro));
  ro.nlayers = o.nlayers;
  RefineCfg cfg;
  if (int r = refine_check_fit(who, ro, F, free_cols, lo, hi, cfg)) return r;
  if (!opt) return fail(SPART_ERR_INVALID, "%s: opt is null", who);
  if (int r = refine_check_band_model(who, o.band_model)) return r;
  if (!(o.rel_step >= 0.0) || !(o.rel_step <= VJP_MAX_REL_STEP))
    return fail(SPART_ERR_INVALID, "%s: rel_step = %g, expected 0 (the default %g) or a finite value in (0, %g]", who, o.rel_step,
                VJP_REL_STEP, VJP_MAX_REL_STEP);
  if (!gy) return fail(SPART_ERR_INVALID, "%s: gy is null", who);
  const int ngy = (gy[0] != nullptr) + (gy[1] != nullptr) + (gy[2] != nullptr);
  if (ngy == 0) return fail(SPART_ERR_INVALID, "%s: every entry of gy is null", who);
  if (o.band_model == 1 && ngy != 1)
    return fail(SPART_ERR_INVALID, "%s: band_model = 1 takes exactly one entry of gy, %d given (one SRF column per forward call)", who,
                ngy);
  if (!grad) return fail(SPART_ERR_INVALID, "%s: grad is null", who);
  if (M < 0 || M > 2000000000LL) return fail(SPART_ERR_INVALID, "%s: M = %lld, expected 0 <= M <= 2e9", who, (long long)M);
  if (M > 0) {
    if (!base) return fail(SPART_ERR_INVALID, "%s: base is null", who);
    if (int i = first_null(base, SPART_NPARAM); i < SPART_NPARAM) return fail(SPART_ERR_INVALID, "%s: base[%d] is null", who, i);
  }
  const double rel = o.rel_step == 0.0 ? VJP_REL_STEP : o.rel_step;
  VjpLayout l;
  return fit_tail(
      who, ctx, M, workspace, workspace_bytes, stream,
      [&](size_t& total) {
        l = vjp_layout(ctx->nb, M, F);
        total = l.total;
        return SPART_OK;
      },
      [&](hipStream_t st) {
        for (int p = 0; p < SPART_NPARAM; ++p) cfg.base[p] = base[p];
        for (int f = 0; f < F; ++f) cfg.freebase[f] = base[cfg.free_col[f]], cfg.h[f] = rel * (cfg.hi[f] - cfg.lo[f]);
        const int column = gy[0] ? 0 : gy[1] ? 1 : 2;         // (what the SRF band model evaluates: its one entry)
        return vjp_impl(ctx, cfg, M, F, gy, column, o, grad, (char*)workspace, l, st);
      });
}

// ---- spart_sample (csrc/spart_sample.h).  Workspace: ONE chunk of Mc = min(M, sample_chunk(W)) observations -- the forward
// block of R = Mc W / 2 rows of a half-step -- then the chunk's state and the per-row hand-over between k_sample_table and
// k_sample_step.
struct SampleLayout {
  int64_t mcap;                 // observations per chunk
  ForwardBlock b;
  size_t x, c, x0, S, Q, bx, bc, na, dead, zp, u2, inside, free_col, out, total;
};
static SampleLayout sample_layout(int nb, int64_t M, int F, int W) {
  SampleLayout l;
  l.mcap = std::min<int64_t>(M, sample_chunk(W));
  const size_t mc = (size_t)l.mcap, rows = mc * (size_t)(W / 2);
  Carver c;
  l.b = forward_block(c, nb, rows, carve_bound_f64((int64_t)rows));
  l.x = c.take(mc * (size_t)W * F * 8);
  l.c = c.take(mc * (size_t)W * 8);
  l.x0 = c.take(mc * F * 8);
  l.S = c.take(mc * F * 8);
  l.Q = c.take(mc * (size_t)refine_ntri(F) * 8);
  l.bx = c.take(mc * F * 8);
  l.bc = c.take(mc * 8);
  l.na = c.take(mc * 8);
  l.dead = c.take(mc * 4);
  l.zp = c.take(rows * 8);
  l.u2 = c.take(rows * 8);
  l.inside = c.take(rows * 4);
  l.free_col = c.take(REFINE_MAXF * 4);
  l.out = c.take(sizeof(SampleOut));
  l.total = c.o;
  return l;
}

size_t spart_sample_workspace_bytes(const spart_ctx* ctx, int64_t M, int F, int W) {
  return fit_sizes_ok(ctx, M, F) && sample_walkers_ok(W, F) ? sample_layout(ctx->nb, M, F, W).total : 0;
}

// the chunk loop: per chunk k_sample_init, then for the start and every step, per half: the table, the forward call, the step
static int sample_impl(spart_ctx* ctx, const SampleCfg& cfg, int64_t M, int F, const double* obs, const double* weights,
                       const spart_sample_opt& o, const SampleOut& out, char* wsp, const SampleLayout& l, hipStream_t st) {
  const int nb = ctx->nb, W = o.W, H = W / 2;
  const Forward fwd(ctx, wsp, l.b, o.column, o.band_model == 1, o.fast_prelude, o.nlayers);
  double* table = fwd.table;
  const SampleState state = {(double*)(wsp + l.x),  (double*)(wsp + l.c),      (double*)(wsp + l.x0),    (double*)(wsp + l.S),
                             (double*)(wsp + l.Q),  (double*)(wsp + l.bx),     (double*)(wsp + l.bc),    (int64_t*)(wsp + l.na),
                             (int32_t*)(wsp + l.dead), (double*)(wsp + l.zp),  (double*)(wsp + l.u2),    (int32_t*)(wsp + l.inside),
                             (int32_t*)(wsp + l.free_col), (SampleOut*)(wsp + l.out)};
  const int64_t n_keep = (o.n_steps - o.burn) / o.thin;
  for (int64_t m0 = 0; m0 < M; m0 += l.mcap) {
    const int mc = (int)std::min<int64_t>(l.mcap, M - m0);
    const int64_t rows = (int64_t)mc * H;
    const uint64_t g0 = (uint64_t)o.obs_offset + (uint64_t)m0;
    const SampleOut oc = {rows_at(out.mean, m0, F),     rows_at(out.cov, m0, F * F),            rows_at(out.std, m0, F),
                          rows_at(out.best_x, m0, F),   rows_at(out.best_cost, m0, 1),          rows_at(out.n_accept, m0, 1),
                          rows_at(out.status, m0, 1),   rows_at(out.chain, m0, n_keep * W * F), rows_at(out.chain_cost, m0, n_keep * W),
                          rows_at(out.last, m0, W * F), rows_at(out.last_cost, m0, W)};
    hipLaunchKernelGGL(k_sample_init, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, cfg, m0, mc, F, W, o.seed, g0,
                       (uint64_t)o.step0, o.rel_init, o.init_radius, o.init, table, state, oc);
    HIP_TRY(hipGetLastError());
    SampleStep a;
    a.cols = fwd.y;
    a.obs = obs + m0 * nb;
    a.wts = rows_at(weights, m0, nb, o.weights_per_obs);
    a.pmu = rows_at(o.prior_mean, m0, F, o.prior_per_obs);
    a.ppw = rows_at(o.prior_weight, m0, F, o.prior_per_obs);
    a.table = table;
    a.Mc = mc, a.F = F, a.nb = nb, a.W = W, a.wper = o.weights_per_obs ? 1 : 0, a.pper = o.prior_per_obs ? 1 : 0;
    a.n_keep = n_keep;
    a.two_tau = 2.0 * o.temperature;
    a.n = (double)(n_keep * W);
    a.st = state;
    for (int64_t rel = 0; rel <= o.n_steps; ++rel) {
      a.start = rel == 0 ? 1 : 0;
      a.last = rel == o.n_steps ? 1 : 0;
      a.keep = rel == 0 ? -1 : sample_keep(rel, o.burn, o.thin);
      for (int h = 0; h < 2; ++h) {
        a.h = h;
        hipLaunchKernelGGL(k_sample_table, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, cfg, mc, F, W, h, a.start, o.seed,
                           g0, (uint64_t)(o.step0 + rel), o.a, table, state);
        HIP_TRY(hipGetLastError());
        if (int rc = fwd.run(rows, st)) return rc;
        hipLaunchKernelGGL(k_sample_step, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
      }
    }
  }
  return SPART_OK;
}

// spart_sobol's checks of F and the host arrays, spart_refine's check of the fit (refine_check_fit), then the sampler's own
// options in the header's order, M, what is NULL with M > 0, the sensor, the workspace
int spart_sample(spart_ctx* ctx, int64_t M, const double* const base[SPART_NPARAM], int F, const int32_t* free_cols, const double* lo,
                 const double* hi, const double* obs, const double* weights, const spart_sample_opt* opt, const spart_sample_out* out,
                 void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_sample";
  if (int r = fit_check_head(who, ctx, F, free_cols, lo, hi)) return r;
  spart_sample_opt o;
  std::memset(&o, 0, sizeof(o));
  if (opt) o = *opt;
  spart_refine_opt ro;
  std::memset(&ro, 0, sizeof(ro));
  ro.column = o.column, ro.nlayers = o.nlayers, ro.prior_per_obs = o.prior_per_obs;
  ro.prior_mean = o.prior_mean, ro.prior_weight = o.prior_weight;
  RefineCfg rc;
  if (int r = refine_check_fit(who, ro, F, free_cols, lo, hi, rc)) return r;
  if (int r = refine_check_band_model(who, o.band_model)) return r;
  if (!sample_walkers_ok(o.W, F))
    return fail(SPART_ERR_INVALID, "%s: W = %d, expected 8, 16, 32 or 64 and W >= 2 F = %d", who, o.W, 2 * F);
  if (o.n_steps < 1 || o.n_steps > SAMPLE_MAX_STEPS || o.burn < 0 || o.burn > o.n_steps - 1 || o.thin < 1 ||
      (o.n_steps - o.burn) / o.thin < 1)
    return fail(SPART_ERR_INVALID, "%s: n_steps = %lld, burn = %lld, thin = %lld: expected 1 <= n_steps <= %d, 0 <= burn < n_steps, "
                "thin >= 1 and (n_steps - burn) / thin >= 1", who, (long long)o.n_steps, (long long)o.burn, (long long)o.thin,
                SAMPLE_MAX_STEPS);
  if (o.a == 0.0) o.a = 2.0;
  if (!std::isfinite(o.a) || !(o.a > 1.0)) return fail(SPART_ERR_INVALID, "%s: a must be finite and > 1 (0 = the default 2.0)", who);
  if (o.temperature == 0.0) o.temperature = 1.0;
  if (!std::isfinite(o.temperature) || !(o.temperature > 0.0))
    return fail(SPART_ERR_INVALID, "%s: temperature must be finite and > 0 (0 = the default 1.0)", who);
  if (o.rel_init == 0.0) o.rel_init = 0.01;
  if (!std::isfinite(o.rel_init) || !(o.rel_init > 0.0))
    return fail(SPART_ERR_INVALID, "%s: rel_init must be finite and > 0 (0 = the default 0.01)", who);
  if (o.step0 < 0 || o.obs_offset < 0)
    return fail(SPART_ERR_INVALID, "%s: step0 = %lld and obs_offset = %lld must be >= 0", who, (long long)o.step0, (long long)o.obs_offset);
  if (M < 0 || M > 2000000000LL) return fail(SPART_ERR_INVALID, "%s: M = %lld, expected 0 <= M <= 2e9", who, (long long)M);
  if (M > 0) {
    if (int r = fit_check_given(who, opt, out, base)) return r;
    if (!obs) return fail(SPART_ERR_INVALID, "%s: obs is null", who);
    if (o.weights_per_obs && !weights) return fail(SPART_ERR_INVALID, "%s: weights_per_obs without weights", who);
    if (!out->mean && !out->cov && !out->std && !out->best_x && !out->best_cost && !out->n_accept && !out->status && !out->chain &&
        !out->chain_cost && !out->last && !out->last_cost)
      return fail(SPART_ERR_INVALID, "%s: every output is null", who);
  }
  SampleLayout l;
  return fit_tail(
      who, ctx, M, workspace, workspace_bytes, stream,
      [&](size_t& total) {
        l = sample_layout(ctx->nb, M, F, o.W);
        total = l.total;
        return SPART_OK;
      },
      [&](hipStream_t st) {
        SampleCfg cfg = fit_cfg<SampleCfg>(rc, base, F);
        for (int f = 0; f < F; ++f) cfg.freebase[f] = base[rc.free_col[f]];
        const SampleOut so = {out->mean,   out->cov,   out->std,        out->best_x, out->best_cost, out->n_accept,
                              out->status, out->chain, out->chain_cost, out->last,   out->last_cost};
        return sample_impl(ctx, cfg, M, F, obs, weights, o, so, (char*)workspace, l, st);
      });
}

int spart_profile_enable(spart_ctx* ctx, int max_calls) {
  if (!ctx) return fail(SPART_ERR_INVALID, "spart_profile_enable: null context");
  DeviceGuard guard(ctx->device);
  std::lock_guard<std::mutex> lock(ctx->mu);
  ctx->profile = max_calls > 0;
  ctx->ev_used = 0;
  ctx->ev_forked.clear();
  while (ctx->ev.size() < (size_t)(max_calls > 0 ? NEV * max_calls : 0)) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    ctx->ev.push_back(e);
  }
  return SPART_OK;
}

int spart_profile_read_stages(spart_ctx* ctx, double stage_ms[SPART_NSTAGE], int* ncalls) {
  if (!ctx || !stage_ms || !ncalls) return fail(SPART_ERR_INVALID, "spart_profile_read_stages: null argument");
  DeviceGuard guard(ctx->device);
  std::lock_guard<std::mutex> lock(ctx->mu);
  static_assert(SPART_NSTAGE + 1 == NEV, "one event more than stages");
  for (int k = 0; k < SPART_NSTAGE; ++k) stage_ms[k] = 0.0;
  int n = 0;
  for (size_t i = 0; i + NEV <= ctx->ev_used; i += NEV) {
    HIP_TRY(hipEventSynchronize(ctx->ev[i + 2]));
    HIP_TRY(hipEventSynchronize(ctx->ev[i + NEV - 1]));
    // events: 0 before the prelude, 1 after it, 2 after the full-band kernel, 3 after the column kernel.  When 3 was
    // recorded on the side stream the column kernel started at event 1, beside the band kernel.
    const bool forked = n < (int)ctx->ev_forked.size() && ctx->ev_forked[n];
    const int from[SPART_NSTAGE] = {0, 1, forked ? 1 : 2}, to[SPART_NSTAGE] = {1, 2, 3};
    for (int k = 0; k < SPART_NSTAGE; ++k) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[i + from[k]], ctx->ev[i + to[k]]));
      stage_ms[k] += ms;
    }
    ++n;
  }
  ctx->ev_used = 0;
  ctx->ev_forked.clear();
  *ncalls = n;
  return SPART_OK;
}

int spart_profile_read(spart_ctx* ctx, double* total_ms, int* ncalls) {
  if (!ctx || !total_ms || !ncalls) return fail(SPART_ERR_INVALID, "spart_profile_read: null argument");
  double st[SPART_NSTAGE];
  int rc = spart_profile_read_stages(ctx, st, ncalls);
  *total_ms = st[1];
  return rc;
}

int spart_calculate_tav(double alpha_deg, const double* nr, int64_t n, double* out) {
  if (!nr || !out || n < 0) return fail(SPART_ERR_INVALID, "spart_calculate_tav: null pointer or negative length");
  for (int64_t i = 0; i < n; ++i) out[i] = calculate_tav(alpha_deg, nr[i]);
  return SPART_OK;
}

int spart_srf_support(const double* wl_srf, const double* p_srf, int32_t nsrf, int32_t nb, int32_t* start, int32_t* ev,
                      double* q, double* Q) {
  if (!wl_srf || !p_srf || !start || nsrf <= 0 || nb <= 0 || (ev == nullptr) != (q == nullptr))
    return fail(SPART_ERR_INVALID, "spart_srf_support: null pointer, a size <= 0, or only one of ev / q given");
  std::vector<double> acc(NEVAL);
  std::vector<char> seen(NEVAL);
  int32_t n = 0;
  for (int32_t j = 0; j < nb; ++j) {
    std::fill(acc.begin(), acc.end(), 0.0);
    std::fill(seen.begin(), seen.end(), 0);
    double tot = 0.0;
    for (int32_t i = 0; i < nsrf; ++i) {
      const double p = p_srf[(size_t)i * nb + j];
      const int g = srf_grid_index(wl_srf[(size_t)i * nb + j]);
      const int e = g < NWL ? g : NWL;                  // the 161 thermal pad bands are ONE evaluation
      acc[e] += p;
      seen[e] = 1;
      tot += p;
    }
    start[j] = n;
    for (int e = 0; e < NEVAL; ++e) {
      if (!seen[e]) continue;
      if (ev) { ev[n] = e; q[n] = acc[e]; }
      ++n;
    }
    if (Q && ev) Q[j] = tot;
  }
  start[nb] = n;
  return SPART_OK;
}

size_t spart_workspace_bytes(const spart_ctx* ctx, int dtype, int64_t B) {
  if (!ctx || B <= 0) return 0;
  return carve(dtype, B).total;
}

int spart_workspace_bandsum(const spart_ctx* ctx, int dtype, int64_t B, size_t* offset, int64_t* nchunk, int* row_stride) {
  if (!ctx || !offset || !nchunk || !row_stride) return fail(SPART_ERR_INVALID, "spart_workspace_bandsum: null argument");
  if (dtype != SPART_F32 && dtype != SPART_F64) return fail(SPART_ERR_INVALID, "spart_workspace_bandsum: bad dtype %d", dtype);
  if (B <= 0 || B > SPART_MAX_BATCH) return fail(SPART_ERR_INVALID, "spart_workspace_bandsum: batch %lld", (long long)B);
  const Workspace ws = carve(dtype, B);            // (one row per workgroup column of k_bands)
  *offset = ws.bs_off;
  *nchunk = ws.nchunk;
  *row_stride = NTILE * TILE;
  return SPART_OK;
}

int spart_prospect_batch(spart_ctx* ctx, int dtype, int64_t B, const double* const leaf[9], void* refl, void* tran,
                         void* kchl, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_prospect_batch";
  Workspace ws;
  if (int rc = gate(ctx, who, dtype, B, workspace, workspace_bytes, ws); rc || B == 0) return rc;
  if (!leaf) return fail(SPART_ERR_INVALID, "%s: null leaf", who);
  if (int i = first_null(leaf, 9); i < 9) return fail(SPART_ERR_INVALID, "%s: leaf[%d] is null", who, i);
  return stage_call(ctx, who, dtype, B, param_slice(0, leaf, 9), PRE_LEAF, ctx->po, workspace, ws, stream,
                    [&](auto t, auto nt, hipStream_t st, auto tab, auto cst) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_prospect<T, nt>), dim3(xcd_grid(ws.nchunk)), dim3(TILE), 0, st, tab, cst, ws.Bp, B, ws.chunk, ctx->po,
                       (T*)refl, (T*)tran, (T*)kchl);
  });
}

int spart_bsm_batch(spart_ctx* ctx, int dtype, int64_t B, const double* const soil[6], const void* rdry_in, void* refl,
                    void* refl_dry, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_bsm_batch";
  Workspace ws;
  if (int rc = gate(ctx, who, dtype, B, workspace, workspace_bytes, ws); rc || B == 0) return rc;
  if (!soil) return fail(SPART_ERR_INVALID, "%s: null soil", who);
  for (int i = 0; i < 6; ++i)
    if (!soil[i] && !may_be_null(9 + i, rdry_in, false)) return fail(SPART_ERR_INVALID, "%s: soil[%d] is null", who, i);
  return stage_call(ctx, who, dtype, B, param_slice(9, soil, 6), PRE_SOIL, ctx->po, workspace, ws, stream,
                    [&](auto t, auto nt, hipStream_t st, auto tab, auto cst) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_bsm<T, nt>), dim3(xcd_grid(ws.nchunk)), dim3(TILE), 0, st, tab, cst, ws.Bp, B, ws.chunk, ctx->po,
                       (const T*)rdry_in, (T*)refl, (T*)refl_dry);
  });
}

int spart_lidf_batch(spart_ctx* ctx, int64_t B, const double* LIDFa, const double* LIDFb, double* lidf, void* stream) {
  if (!ctx) return fail(SPART_ERR_INVALID, "spart_lidf_batch: null context");
  if (B < 0 || !LIDFa || !LIDFb || !lidf) return fail(SPART_ERR_INVALID, "spart_lidf_batch: bad argument");
  if (B == 0) return SPART_OK;
  DeviceGuard guard(ctx->device);
  hipLaunchKernelGGL(k_lidf, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, LIDFa, LIDFb, B, lidf);
  HIP_TRY(hipGetLastError());
  return SPART_OK;
}

int spart_sailh_batch(spart_ctx* ctx, int dtype, int64_t B, const void* rho, const void* tau, const void* rs,
                      const double* const canopy[4], const double* const angles[3], const double* lidf_in, int32_t nlayers,
                      void* const out4[4], void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_sailh_batch";
  Workspace ws;
  if (int rc = gate(ctx, who, dtype, B, workspace, workspace_bytes, ws); rc || B == 0) return rc;
  if (!rho || !tau || !rs || !canopy || !angles || !out4) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  if (nlayers < 0 || nlayers > SPART_MAX_NLAYERS)
    return fail(SPART_ERR_INVALID, "%s: nlayers = %d (0 = the default 60, else 1 ... %d)", who, nlayers, SPART_MAX_NLAYERS);
  for (int i = 0; i < 4; ++i)
    if ((!canopy[i] && !may_be_null(15 + i, false, lidf_in)) || !out4[i])
      return fail(SPART_ERR_INVALID, "%s: canopy/out4[%d] is null", who, i);
  if (int i = first_null(angles, 3); i < 3) return fail(SPART_ERR_INVALID, "%s: angles[%d] is null", who, i);
  ParamPtrs pp = param_slice(15, canopy, 4);
  for (int i = 0; i < 3; ++i) pp.p[19 + i] = angles[i];
  pp.lidf = lidf_in;
  pp.nlayers = nlayers;
  return stage_call(ctx, who, dtype, B, pp, PRE_CANOPY, ctx->pf, workspace, ws, stream,
                    [&](auto t, auto nt, hipStream_t st, auto, auto cst) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_sailh<T, nt>), dim3((unsigned)(ws.nchunk * NTILE_FULL)), dim3(TILE), 0, st, cst, ws.Bp, B, ws.chunk,
                       ctx->pf, (const T*)rho, (const T*)tau, (const T*)rs, (T*)out4[0], (T*)out4[1], (T*)out4[2], (T*)out4[3]);
  });
}

int spart_products(spart_ctx* ctx, int64_t B, const double* const params[SPART_NPARAM], const spart_products_out* out,
                   void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_products";
  constexpr int NREAD = 22;                         // params[22 ... 26] (atmosphere, DOY) are not read
  Workspace ws;
  if (int rc = gate(ctx, who, SPART_F64, B, workspace, workspace_bytes, ws); rc) return rc;
  if (!out) return fail(SPART_ERR_INVALID, "%s: null out", who);
  if (B == 0) return SPART_OK;
  if (!out->fapar_bs && !out->fapar_ws && !out->albedo_bs && !out->albedo_ws && !out->fcover)
    return fail(SPART_ERR_INVALID, "%s: every output is null", who);
  if (!params) return fail(SPART_ERR_INVALID, "%s: null params", who);
  if (int i = first_null(params, NREAD); i < NREAD) return fail(SPART_ERR_INVALID, "%s: params[%d] is null", who, i);
  const ProductsOut po{out->fapar_bs, out->fapar_ws, out->albedo_bs, out->albedo_ws, out->fcover};
  return stage_call(ctx, who, SPART_F64, B, param_slice(0, params, NREAD), PRE_LEAF | PRE_SOIL | PRE_CANOPY, ctx->po, workspace,
                    ws, stream, [&](auto t, auto, hipStream_t st, auto tab, auto cst) {
    if constexpr (std::is_same_v<decltype(t), double>)
      hipLaunchKernelGGL(k_products, dim3((unsigned)((B + 63) / 64)), dim3(64 * COL_WAVES), 0, st, tab, cst, ws.Bp,
                         (const double*)ctx->Ea, ctx->ea_par, ctx->ea_all, params[16], params[17], B, po);
  });
}

int spart_smac_batch(spart_ctx* ctx, int64_t B, const double* const angles[3], const double* const atm[4],
                     double* const out9[9], void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_smac_batch";
  Workspace ws;
  if (int rc = gate(ctx, who, SPART_F64, B, workspace, workspace_bytes, ws); rc || B == 0) return rc;
  if (ctx->nb == 0) return fail(SPART_ERR_NOSENSOR, "%s: context has no sensor", who);
  if (!angles || !atm || !out9) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  if (int i = first_null(angles, 3); i < 3) return fail(SPART_ERR_INVALID, "%s: angles[%d] is null", who, i);
  if (int i = first_null(atm, 4); i < 4) return fail(SPART_ERR_INVALID, "%s: atm[%d] is null", who, i);
  if (int i = first_null(out9, 9); i < 9) return fail(SPART_ERR_INVALID, "%s: out9[%d] is null", who, i);
  return guarded(ctx, who, workspace, ws.total, stream, [&](hipStream_t st) -> int {
    ParamPtrs pp = param_slice(19, angles, 3);
    for (int i = 0; i < 4; ++i) pp.p[22 + i] = atm[i];
    double* a = (double*)((char*)workspace + ws.atm_off);
    int rc = launch_prelude(false, pp, PRE_ATM, B, ws.Bp, nullptr, nullptr, a, st);
    if (rc) return rc;
    Out9 o;
    for (int i = 0; i < 9; ++i) o.o[i] = out9[i];
    int64_t n = B * ctx->nb;
    hipLaunchKernelGGL(k_smac, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)ctx->coef, ctx->nb,
                       (const double*)a, ws.Bp, B, o);
    HIP_TRY(hipGetLastError());
    return SPART_OK;
  });
}

int spart_run_batch(spart_ctx* ctx, int dtype, int64_t B, const double* const params[SPART_NPARAM],
                    const double* rho_thermal, const double* tau_thermal, void* R_TOC, void* R_TOA, void* L_TOA,
                    const spart_materialize* opt, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_run_batch";
  Workspace ws;
  if (int rc = gate(ctx, who, dtype, B, workspace, workspace_bytes, ws); rc || B == 0) return rc;
  if (ctx->nb == 0) return fail(SPART_ERR_NOSENSOR, "%s: context has no sensor", who);
  if (!params || !R_TOC || !R_TOA || !L_TOA) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  for (int i = 0; i < SPART_NPARAM; ++i)
    if (!params[i] && !may_be_null(i, opt && opt->rdry_in, opt && opt->lidf_in))
      return fail(SPART_ERR_INVALID, "%s: params[%d] is null", who, i);
  if (opt && (opt->nlayers < 0 || opt->nlayers > SPART_MAX_NLAYERS))
    return fail(SPART_ERR_INVALID, "%s: nlayers = %d (0 = the default 60, else 1 ... %d)", who, opt->nlayers, SPART_MAX_NLAYERS);
  if (dtype == SPART_F64 && opt && opt->f32_bands &&
      (opt->leaf_refl || opt->leaf_tran || opt->leaf_kchl || opt->soil_refl || opt->soil_refl_dry || opt->rso || opt->rdo ||
       opt->rsd || opt->rdd || opt->band_mean || opt->rdry_in || opt->f32_columns))
    // float64 columns (identical to the float64 mode's) over a float32 full-band pass: nothing the float32 kernel
    // would have to write in float64 may be requested
    return fail(SPART_ERR_INVALID, "%s: f32_bands goes with the sensor columns (and rsoil / La) only", who);
  if (wants_srf(opt) && opt->f32_columns)
    return fail(SPART_ERR_INVALID, "%s: the SRF-convolved outputs come from the float64 column path; they do not go with f32_columns", who);
  return guarded(ctx, who, workspace, ws.total, stream, [&](hipStream_t st) {
    char* wsp = (char*)workspace;
    if (dtype == SPART_F64 && opt && opt->f32_bands)
      return run_impl<float, double, double>(ctx, B, params, rho_thermal, tau_thermal, R_TOC, R_TOA, L_TOA, opt, wsp, ws, st);
    if (dtype == SPART_F64)
      return run_impl<double, double, double>(ctx, B, params, rho_thermal, tau_thermal, R_TOC, R_TOA, L_TOA, opt, wsp, ws, st);
    return (opt && opt->f32_columns)
               ? run_impl<float, float, float>(ctx, B, params, rho_thermal, tau_thermal, R_TOC, R_TOA, L_TOA, opt, wsp, ws, st)
               : run_impl<float, double, float>(ctx, B, params, rho_thermal, tau_thermal, R_TOC, R_TOA, L_TOA, opt, wsp, ws, st);
  });
}

size_t spart_lut_workspace_bytes(int dtype, int64_t B, int nb, int64_t M) {
  return lut_sizes_ok(LUT_NEAREST, dtype, B, nb, M, 0) ? lut_layout(dtype, B, nb, M).total : 0;
}

int spart_lut_nearest(spart_ctx* ctx, int dtype, int64_t B, int nb, const void* lut, int64_t M, const void* obs,
                      const void* weights, int64_t* best_idx, void* best_cost, void* workspace, size_t workspace_bytes,
                      void* stream) {
  return lut_search(ctx, LUT_NEAREST, dtype, B, nb, lut, M, obs, weights, 0, best_idx, best_cost, workspace, workspace_bytes,
                    spart_lut_workspace_bytes(dtype, B, nb, M), stream, [&](auto t, char* wsp, hipStream_t st) {
                      return lut_impl<decltype(t)>(ctx, dtype, B, nb, lut, M, obs, weights, best_idx, best_cost, wsp, st);
                    });
}

int spart_lut_stats(spart_ctx* ctx, int dtype, int64_t B, int nb, int64_t M, const void* workspace, int64_t* n_brute_force,
                    double* nmax) {
  int64_t* const counts[] = {n_brute_force};
  return lut_read_stats(ctx, "spart_lut_stats", dtype, workspace, spart_lut_workspace_bytes(dtype, B, nb, M) != 0,
                        [&] { return lut_layout(dtype, B, nb, M).ctl; }, counts, 1, nmax);
}

size_t spart_lut_topk_workspace_bytes(int dtype, int64_t B, int nb, int64_t M, int k) {
  return lut_sizes_ok(LUT_TOPK, dtype, B, nb, M, k) ? lut_topk_layout(dtype, B, nb, M, k).total : 0;
}

int spart_lut_topk(spart_ctx* ctx, int dtype, int64_t B, int nb, const void* lut, int64_t M, const void* obs, const void* weights,
                   int k, int64_t* idx, void* cost, void* workspace, size_t workspace_bytes, void* stream) {
  return lut_search(ctx, LUT_TOPK, dtype, B, nb, lut, M, obs, weights, k, idx, cost, workspace, workspace_bytes,
                    spart_lut_topk_workspace_bytes(dtype, B, nb, M, k), stream, [&](auto t, char* wsp, hipStream_t st) {
                      return lut_topk_impl<decltype(t)>(dtype, B, nb, lut, M, obs, weights, k, idx, cost, wsp, st);
                    });
}

int spart_lut_topk_stats(spart_ctx* ctx, int dtype, int64_t B, int nb, int64_t M, int k, const void* workspace,
                         int64_t* n_brute_force, int64_t* n_candidates, int64_t* max_candidates, double* nmax) {
  int64_t* const counts[] = {n_brute_force, n_candidates, max_candidates};
  return lut_read_stats(ctx, "spart_lut_topk_stats", dtype, workspace, spart_lut_topk_workspace_bytes(dtype, B, nb, M, k) != 0,
                        [&] { return lut_topk_layout(dtype, B, nb, M, k).ctl; }, counts, 3, nmax);
}

size_t spart_lut_topk_wide_workspace_bytes(int dtype, int64_t B, int nb, int64_t M, int k) {
  return lut_sizes_ok(LUT_WIDE, dtype, B, nb, M, k) ? lut_wide_layout(dtype, B, nb, M, k, false).total : 0;
}

int spart_lut_topk_wide(spart_ctx* ctx, int dtype, int64_t B, int nb, const void* lut, int64_t M, const void* obs,
                        const void* weights, int k, int64_t* idx, void* cost, void* workspace, size_t workspace_bytes,
                        void* stream) {
  return lut_search(ctx, LUT_WIDE, dtype, B, nb, lut, M, obs, weights, k, idx, cost, workspace, workspace_bytes,
                    spart_lut_topk_wide_workspace_bytes(dtype, B, nb, M, k), stream, [&](auto t, char* wsp, hipStream_t st) {
                      using T = decltype(t);
                      return lut_wide_impl<T, false>(dtype, B, nb, lut, M, obs, weights, k, k, 0.0, true, wsp, st,
                                                    lutw_topk_consumer<T, false>((const T*)lut, (const T*)obs, (const T*)weights,
                                                                                nb, B, M, k, idx, cost));
                    });
}

int spart_lut_topk_wide_stats(spart_ctx* ctx, int dtype, int64_t B, int nb, int64_t M, int k, const void* workspace,
                              int64_t* n_brute_force, int64_t* n_candidates, int64_t* max_candidates, double* nmax) {
  int64_t* const counts[] = {n_brute_force, n_candidates, max_candidates};
  return lut_read_stats(ctx, "spart_lut_topk_wide_stats", dtype, workspace,
                        spart_lut_topk_wide_workspace_bytes(dtype, B, nb, M, k) != 0,
                        [&] { return lut_wide_layout(dtype, B, nb, M, k, false).ctl; }, counts, 3, nmax);
}

size_t spart_lut_topk_obs_weights_workspace_bytes(int dtype, int64_t B, int nb, int64_t M, int k) {
  return lut_sizes_ok(LUT_OBSW, dtype, B, nb, M, k) ? lut_wide_layout(dtype, B, nb, M, k, true).total : 0;
}

int spart_lut_topk_obs_weights(spart_ctx* ctx, int dtype, int64_t B, int nb, const void* lut, int64_t M, const void* obs,
                               const void* weights, int k, int64_t* idx, void* cost, void* workspace, size_t workspace_bytes,
                               void* stream) {
  return lut_search(ctx, LUT_OBSW, dtype, B, nb, lut, M, obs, weights, k, idx, cost, workspace, workspace_bytes,
                    spart_lut_topk_obs_weights_workspace_bytes(dtype, B, nb, M, k), stream, [&](auto t, char* wsp, hipStream_t st) {
                      using T = decltype(t);
                      return lut_wide_impl<T, true>(dtype, B, nb, lut, M, obs, weights, k, k, 0.0, true, wsp, st,
                                                    lutw_topk_consumer<T, true>((const T*)lut, (const T*)obs, (const T*)weights,
                                                                                nb, B, M, k, idx, cost));
                    });
}

int spart_lut_topk_obs_weights_stats(spart_ctx* ctx, int dtype, int64_t B, int nb, int64_t M, int k, const void* workspace,
                                     int64_t* n_brute_force, int64_t* n_candidates, int64_t* max_candidates, double* nbound) {
  int64_t* const counts[] = {n_brute_force, n_candidates, max_candidates};
  return lut_read_stats(ctx, "spart_lut_topk_obs_weights_stats", dtype, workspace,
                        spart_lut_topk_obs_weights_workspace_bytes(dtype, B, nb, M, k) != 0,
                        [&] { return lut_wide_layout(dtype, B, nb, M, k, true).ctl; }, counts, 3, nbound);
}

// The posterior shares the per-observation-weights layout of a k = LUT_BAYES_CAPK search: same chunks, same flag list.
static bool lut_bayes_sizes_ok(int dtype, int64_t B, int nb, int64_t M) {
  return lut_sizes_ok(LUT_OBSW, dtype, B, nb, M, LUT_BAYES_CAPK) && B <= 2000000000LL && M <= 2000000000LL;
}

size_t spart_lut_bayes_workspace_bytes(int dtype, int64_t B, int nb, int64_t M) {
  return lut_bayes_sizes_ok(dtype, B, nb, M) ? lut_wide_layout(dtype, B, nb, M, LUT_BAYES_CAPK, true).total : 0;
}

// (lut_search's checks and order, with the parameter table, the options and the output struct; an empty LUT is an answer here)
int spart_lut_bayes(spart_ctx* ctx, int dtype, int64_t B, int nb, const void* lut, int P, const double* params, int64_t M,
                    const void* obs, const void* weights, const spart_lut_bayes_opt* opt, const spart_lut_bayes_out* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_lut_bayes";
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (!dtype_ok(dtype)) return fail(SPART_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  if (B < 0 || M < 0 || !LUT_OBSW.nb_ok(nb) || P < 1 || P > LUT_BAYES_MAXP || B > 2000000000LL || M > 2000000000LL)
    return fail(SPART_ERR_INVALID, "%s: bad sizes (B=%lld M=%lld nb=%d P=%d; 1 <= nb <= %d, 1 <= P <= %d, B and M <= 2e9)", who,
                (long long)B, (long long)M, nb, P, LUT_OBSW.nb_max, LUT_BAYES_MAXP);
  if (!opt || !out) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  if (!(opt->cut >= 0.0)) return fail(SPART_ERR_INVALID, "%s: cut = %g, expected >= 0 (or +inf)", who, opt->cut);
  if (!(opt->temperature >= 0.0) || std::isinf(opt->temperature))
    return fail(SPART_ERR_INVALID, "%s: temperature = %g, expected 0 (= 1.0) or finite > 0", who, opt->temperature);
  if (opt->brute_force != 0 && opt->brute_force != 1)
    return fail(SPART_ERR_INVALID, "%s: brute_force = %d, expected 0 or 1", who, opt->brute_force);
  if (M == 0) return SPART_OK;                         // (the (0,) outputs of an empty batch have no address)
  if (!out->mean && !out->std && !out->sum_w && !out->ess && !out->count && !out->best_idx && !out->best_cost)
    return fail(SPART_ERR_INVALID, "%s: every output is NULL", who);
  const LutBayesOut o = {out->mean, out->std, out->sum_w, out->ess, out->count, out->best_idx, out->best_cost};
  if (B == 0)                                          // no row: every observation gets the empty outputs
    return guarded(ctx, who, nullptr, 0, stream, [&](hipStream_t st) {
      return by_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL((k_lut_bayes_empty<decltype(t)>), dim3((unsigned)(M < 65536 ? M : 65536)), dim3(64), 0, st, M, P, o);
        HIP_TRY(hipGetLastError());
        return SPART_OK;
      });
    });
  if (!lut || !params || !obs || !weights) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  const size_t need = spart_lut_bayes_workspace_bytes(dtype, B, nb, M);
  if (!workspace || workspace_bytes < need)
    return fail(SPART_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
  return guarded(ctx, who, workspace, need, stream, [&](hipStream_t st) {
    return by_dtype(dtype, [&](auto t) {
      return lut_bayes_impl<decltype(t)>(dtype, B, nb, lut, P, params, M, obs, weights, *opt, o, (char*)workspace, st);
    });
  });
}

// (spart_lut_bayes' checks in its order, with the levels behind the NULL check of opt and out and quant as an eighth output)
int spart_lut_bayes_quantiles(spart_ctx* ctx, int dtype, int64_t B, int nb, const void* lut, int P, const double* params, int64_t M,
                              const void* obs, const void* weights, const spart_lut_bayes_q_opt* qopt,
                              const spart_lut_bayes_q_out* qout, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spart_lut_bayes_quantiles";
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (!dtype_ok(dtype)) return fail(SPART_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  if (B < 0 || M < 0 || !LUT_OBSW.nb_ok(nb) || P < 1 || P > LUT_BAYES_MAXP || B > 2000000000LL || M > 2000000000LL)
    return fail(SPART_ERR_INVALID, "%s: bad sizes (B=%lld M=%lld nb=%d P=%d; 1 <= nb <= %d, 1 <= P <= %d, B and M <= 2e9)", who,
                (long long)B, (long long)M, nb, P, LUT_OBSW.nb_max, LUT_BAYES_MAXP);
  if (!qopt || !qout) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  if (qopt->nq < 1 || qopt->nq > LUT_BAYES_MAXQ)
    return fail(SPART_ERR_INVALID, "%s: nq = %d, expected 1 <= nq <= %d", who, qopt->nq, LUT_BAYES_MAXQ);
  if (!qopt->levels) return fail(SPART_ERR_INVALID, "%s: null levels", who);
  LutBayesLevels lv = {};
  lv.nq = qopt->nq;
  for (int i = 0; i < lv.nq; ++i) {
    lv.q[i] = qopt->levels[i];
    if (!(lv.q[i] >= 0.0 && lv.q[i] <= 1.0))
      return fail(SPART_ERR_INVALID, "%s: levels[%d] = %g, expected a level in [0, 1]", who, i, lv.q[i]);
  }
  const spart_lut_bayes_opt* opt = &qopt->base;
  const spart_lut_bayes_out* out = &qout->base;
  if (!(opt->cut >= 0.0)) return fail(SPART_ERR_INVALID, "%s: cut = %g, expected >= 0 (or +inf)", who, opt->cut);
  if (!(opt->temperature >= 0.0) || std::isinf(opt->temperature))
    return fail(SPART_ERR_INVALID, "%s: temperature = %g, expected 0 (= 1.0) or finite > 0", who, opt->temperature);
  if (opt->brute_force != 0 && opt->brute_force != 1)
    return fail(SPART_ERR_INVALID, "%s: brute_force = %d, expected 0 or 1", who, opt->brute_force);
  if (M == 0) return SPART_OK;                         // (the (0,) outputs of an empty batch have no address)
  double* quant = qout->quant;
  if (!out->mean && !out->std && !out->sum_w && !out->ess && !out->count && !out->best_idx && !out->best_cost && !quant)
    return fail(SPART_ERR_INVALID, "%s: every output is NULL", who);
  const LutBayesOut o = {out->mean, out->std, out->sum_w, out->ess, out->count, out->best_idx, out->best_cost};
  if (B == 0)                                          // no row: every observation gets the empty outputs, every quantile NaN
    return guarded(ctx, who, nullptr, 0, stream, [&](hipStream_t st) {
      return by_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL((k_lut_bayes_empty<decltype(t)>), dim3((unsigned)(M < 65536 ? M : 65536)), dim3(64), 0, st, M, P, o);
        HIP_TRY(hipGetLastError());
        if (quant) {
          const int64_t n = M * P * lv.nq, blocks = (n + 255) / 256;
          hipLaunchKernelGGL(k_lut_posterior_quant_empty, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, n, quant);
          HIP_TRY(hipGetLastError());
        }
        return SPART_OK;
      });
    });
  if (!lut || !params || !obs || !weights) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  const size_t need = spart_lut_bayes_workspace_bytes(dtype, B, nb, M);
  if (!workspace || workspace_bytes < need)
    return fail(SPART_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
  return guarded(ctx, who, workspace, need, stream, [&](hipStream_t st) {
    return by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      if (!quant)                                      // no quantile asked for: the call is spart_lut_bayes
        return lut_bayes_impl<T>(dtype, B, nb, lut, P, params, M, obs, weights, *opt, o, (char*)workspace, st);
      return lut_bayes_quant_impl<T>(dtype, B, nb, lut, P, params, M, obs, weights, *opt, o, lv, quant, (char*)workspace, st);
    });
  });
}

int spart_lut_bayes_stats(spart_ctx* ctx, int dtype, int64_t B, int nb, int64_t M, const void* workspace, int64_t* n_brute_force,
                          int64_t* n_candidates, int64_t* max_candidates, double* nbound) {
  int64_t* const counts[] = {n_brute_force, n_candidates, max_candidates};
  return lut_read_stats(ctx, "spart_lut_bayes_stats", dtype, workspace, spart_lut_bayes_workspace_bytes(dtype, B, nb, M) != 0,
                        [&] { return lut_wide_layout(dtype, B, nb, M, LUT_BAYES_CAPK, true).ctl; }, counts, 3, nbound);
}

// (the argument checks of lut_search, in its order, for a call without dtype, bands and workspace)
int spart_lut_summarise(spart_ctx* ctx, int64_t B, int P, const double* params, int64_t M, int k, const int64_t* idx,
                        double* mean, double* median, double* std, int32_t* count, void* stream) {
  const char* who = "spart_lut_summarise";
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (B < 0 || M < 0 || P < 1 || P > LUT_SUM_MAXP || B > 2000000000LL || M > 2000000000LL)
    return fail(SPART_ERR_INVALID, "%s: bad sizes (B=%lld M=%lld P=%d; 1 <= P <= %d, B and M <= 2e9)", who, (long long)B,
                (long long)M, P, LUT_SUM_MAXP);
  if (k < 1 || k > LUT_TOPK_MAXK) return fail(SPART_ERR_INVALID, "%s: k = %d, expected 1 <= k <= %d", who, k, LUT_TOPK_MAXK);
  if (M == 0) return SPART_OK;
  if (B == 0) return fail(SPART_ERR_INVALID, "%s: empty table", who);
  if (!params || !idx || (!mean && !median && !std && !count)) return fail(SPART_ERR_INVALID, "%s: null argument", who);
  return guarded(ctx, who, nullptr, 0, stream,
                 [&](hipStream_t st) { return launch_lut_summarise(B, P, params, M, k, idx, mean, median, std, count, st); });
}

int spart_refine_leaf(spart_ctx* ctx, int64_t M, const double* const leaf[9], int F, const int32_t* free_cols, const double* lo,
                      const double* hi, const double* obs_refl, const double* obs_tran, const double* w_refl, const double* w_tran,
                      const spart_leaf_fit_opt* opt, const spart_leaf_fit_out* out, void* stream) {
  const char* who = "spart_refine_leaf";
  if (!ctx) return fail(SPART_ERR_INVALID, "%s: null context", who);
  if (F < 1 || F > LEAF_MAXF) return fail(SPART_ERR_INVALID, "%s: F = %d, expected 1 <= F <= %d", who, F, LEAF_MAXF);
  if (!free_cols || !lo || !hi) return fail(SPART_ERR_INVALID, "%s: null argument (free_cols, lo and hi are required)", who);
  LeafFitArgs a;
  std::memset(&a, 0, sizeof(a));
  bool is_free[LEAF_NPAR] = {false};
  for (int f = 0; f < F; ++f) {
    const int c = free_cols[f];
    if (c < 0 || c >= LEAF_NPAR) return fail(SPART_ERR_INVALID, "%s: free_cols[%d] = %d, expected 0 ... %d", who, f, c, LEAF_NPAR - 1);
    if (is_free[c]) return fail(SPART_ERR_INVALID, "%s: column %d is free twice", who, c);
    is_free[c] = true;
    a.free_col[f] = c;
  }
  for (int f = 0; f < F; ++f) {
    if (!std::isfinite(lo[f]) || !std::isfinite(hi[f]) || !(lo[f] < hi[f]))
      return fail(SPART_ERR_INVALID, "%s: bounds of free_cols[%d]: finite lo < hi expected", who, f);
    a.lo[f] = lo[f];
    a.hi[f] = hi[f];
  }
  if (!opt) return fail(SPART_ERR_INVALID, "%s: opt is null", who);
  if (opt->n_iter < 0 || opt->n_iter > REFINE_MAX_ITER)
    return fail(SPART_ERR_INVALID, "%s: n_iter = %d, expected 0 ... %d", who, opt->n_iter, REFINE_MAX_ITER);
  if (!(opt->rel_step >= 0.0) || !(opt->lambda0 >= 0.0) || std::isinf(opt->rel_step) || std::isinf(opt->lambda0))
    return fail(SPART_ERR_INVALID, "%s: rel_step and lambda0 must be finite and >= 0 (0 = the default)", who);
  if (opt->weights_per_obs != 0 && opt->weights_per_obs != 1)
    return fail(SPART_ERR_INVALID, "%s: weights_per_obs = %d (0: one row for all, 1: one row per leaf)", who, opt->weights_per_obs);
  if (!opt->prior_mean != !opt->prior_weight)
    return fail(SPART_ERR_INVALID, "%s: prior_mean and prior_weight come together (both NULL = no prior)", who);
  if (opt->prior_per_obs != 0 && opt->prior_per_obs != 1)
    return fail(SPART_ERR_INVALID, "%s: prior_per_obs = %d (0: one row for all, 1: one row per leaf)", who, opt->prior_per_obs);
  if (!obs_refl && !obs_tran) return fail(SPART_ERR_INVALID, "%s: obs_refl and obs_tran are both null", who);
  if ((w_refl && !obs_refl) || (w_tran && !obs_tran))
    return fail(SPART_ERR_INVALID, "%s: weights given for an observation array that is null", who);
  if (!out || !out->x || !out->cost) return fail(SPART_ERR_INVALID, "%s: out, out->x and out->cost are required", who);
  if (M < 0 || M > 2000000000LL) return fail(SPART_ERR_INVALID, "%s: M = %lld, expected 0 <= M <= 2e9", who, (long long)M);
  if (M == 0) return SPART_OK;
  if (!leaf) return fail(SPART_ERR_INVALID, "%s: null leaf", who);
  if (int i = first_null(leaf, LEAF_NPAR); i < LEAF_NPAR) return fail(SPART_ERR_INVALID, "%s: leaf[%d] is null", who, i);
  const double rel = opt->rel_step == 0.0 ? 1e-3 : opt->rel_step;
  for (int k = 0; k < LEAF_NPAR; ++k) a.leaf[k] = leaf[k];
  for (int f = 0; f < F; ++f) a.h[f] = rel * (a.hi[f] - a.lo[f]);
  a.n_iter = opt->n_iter, a.wper = opt->weights_per_obs, a.pper = opt->prior_per_obs;
  a.lambda0 = opt->lambda0 == 0.0 ? 1e-2 : opt->lambda0;
  a.obs_r = obs_refl, a.obs_t = obs_tran, a.w_r = w_refl, a.w_t = w_tran;
  a.pmu = opt->prior_mean, a.ppw = opt->prior_weight;
  a.x = out->x, a.cost = out->cost, a.cost0 = out->cost0, a.sdev = out->std, a.n_accept = out->n_accept;
  a.y_r = out->y_refl, a.y_t = out->y_tran;
  return guarded(ctx, who, nullptr, 0, stream, [&](hipStream_t st) {
    const unsigned blocks = (unsigned)std::min<int64_t>(M, LEAF_MAX_BLOCKS);
    launch_refine_leaf<1>(F, blocks, st, (const double*)ctx->tabD, a, M);
    HIP_TRY(hipGetLastError());
    return SPART_OK;
  });
}

}  // extern "C"
