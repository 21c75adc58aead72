// resnmtf_hip.hip -- host side of libresnmtf_hip.so: handle, device memory, launch schedule,
// hipGraph capture and the C-ABI declared in include/resnmtf_hip.h.
//
// Schedule of one sweep (R/update_steps.r:272-319) for owned views v = 0..V-1, in order, ONE stream:
//   F_v          factor_update<F>   update_f, reads U_v = X_v G_v and the F coefficients
//   pass Xt.F    main workgroups: T_v = X_v^T F_v'   | k x k job kk_f
//   G_v          factor_update<G>   update_g, reads T_v and the G coefficients
//   pass X.G'    main workgroups: U_v = X_v G_v'     | k x k job kk_s
// Every k x k chain (S rule, lambda/mu, error, coefficient matrices) depends only on the factor that
// was just updated; it runs once inside the pass launch that follows that update, while the main
// workgroups stream X: as workgroup 0 fed by the update kernel's fp64 partials (mode A, k <= 16) or
// in the last-arriving MFMA aux workgroup (mode B) -- see resnmtf_kernels.hip.inc.  Cross-view
// coupling (phi/psi: running F/G; xi: running S) is ordered by the stream.  A run starts with one
// X.G launch per view whose kk_s runs in mode 0 (F coefficients from the current S and G).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "resnmtf_hip.h"
#include "resnmtf_kernels.hip.inc"
#include "resnmtf_device_view.hip.inc"
#include "resnmtf_device_factors.hip.inc"
#include "resnmtf_view_readback.hip.inc"
#include "resnmtf_sparse.hip.inc"
#include <rocprim/rocprim.hpp>
#include "resnmtf_sparse_shuffle.hip.inc"
#include "resnmtf_sparse_subsample.hip.inc"
#include "resnmtf_sparse_device_view.hip.inc"
#include "resnmtf_jsd.hip.inc"
#include "resnmtf_group.hip.inc"
#include "resnmtf_bisil_plan.h"
#include "resnmtf_bisil.hip.inc"
#include "resnmtf_split_tu.h"
#include "resnmtf_internal.h"
#include "resnmtf_small_linalg.h"
#ifdef RESNMTF_SPLIT_TU      // product build: the k <= 16 pass lives in resnmtf_pass_k16.hip (its own scheduling strategy)
#define RESNMTF_EXTERN(NW, UNR, XG, MA) extern template __global__ void pass_kernel<1, NW, UNR, XG, MA, 0>(PassArgs, KKFArgs, KKSArgs);
RESNMTF_PASS_K16_LIST(RESNMTF_EXTERN)
#undef RESNMTF_EXTERN
#endif

namespace {

std::string g_create_error;

inline int round_up(int x, int a) { return (x + a - 1) / a * a; }
inline int ceil_div(int x, int a) { return (x + a - 1) / a; }

struct SharedMap {
  bool set = false;        // false or count < 0  ->  NA
  int count = -1;
  int* dev = nullptr;      // [len_v] row of w or -1
  bool identity = false;   // every row of v maps to the same row of w (auto-named views): no lookup needed
};

// One half of a view.  X (n x m) ~ F S G^T has two symmetric halves, and everything that exists once per half lives here
// under one name:
//   side[SIDE_F]: length n, factor F, multiplier lambda, coupling matrix phi, row maps;    fed by the X.G pass
//   side[SIDE_G]: length m, factor G, multiplier mu,     coupling matrix psi, column maps; fed by the Xt.F pass
// THE CROSSOVER (the one place the mapping is easy to get backwards): the pass that feeds side s writes its product slab
// P ([nsplit][pad][KP]) for the update of side s, but its B operand is the factor of the OTHER side, other(s), and the image
// it streams has the lines of side s as its 64-wide tiles and the lines of other(s) as its rows: X.G feeds F, multiplies by
// G and streams X^T (tile-major over the rows of X; sparse: the CSR); Xt.F feeds G, multiplies by F and streams X (the CSC).
// feeds(xg) names the side a pass feeds; index 0 = F matches wchain[g], schain[g] and the [0] = X.G columns of
// resnmtf_view_plan_info.
enum { SIDE_F = 0, SIDE_G = 1 };
inline int other(int s) { return 1 - s; }
inline int feeds(bool xg) { return xg ? SIDE_F : SIDE_G; }

struct Side {
  int len = 0, pad = 0;              // n / m and their multiples of 64
  double* W = nullptr;               // the fp64 factor F / G [len][k]
  float* W32 = nullptr;              // its f32 operand copy
  unsigned short* Wk = nullptr;      // k > 16: its K-packed bf16 pieces (B operand of pass_body_k32)
  double* lm = nullptr;              // lambda / mu
  double *Ma = nullptr, *Md = nullptr;   // the k x k coefficient matrices of the update
  double* part = nullptr;            // mode A: fp64 Gram partials of the update workgroups
  int rpb = 16, nblk = 1;            // rows per update workgroup, update workgroups
  // exchange block (replicate_f / replicate_gs): [xsum | Ma | Md | lm] contiguous -- the update's inputs -- a slice of the
  // handle's arena[s]; xsum = the split slabs of the pass folded into one f32 slab
  void* xblk = nullptr;
  size_t xblk_bytes = 0;
  float* xsum = nullptr;
  bool replica = false;              // non-owned view whose update of this side runs here too
  std::vector<SharedMap> map;        // shared rows / columns, indexed by the other view
  UpdateArgs arg{};
  // ---- the pass that feeds this side
  PassArgs pass{};
  int nsplit = 1, rps = 64, nw = 4, nsaux = 1, rpsaux = 64;
  int tw = 8;                        // k > 16 (wide form): 64-column tiles per workgroup
  bool pp = false;                   // k <= 16, streamed geometry: ping-pong prefetch form of the pass (UNROLL 4)
  float *P = nullptr, *Paux = nullptr;
  int* cnt = nullptr;
  // the dense image it streams, tile-major: tile t (64 lines of this side) is a contiguous [other's pad][64] block; ldx = the
  // TILE stride (floats).  SIDE_F: X^T, SIDE_G: X
  float* X = nullptr;
  size_t ldx = 0, x_floats = 0;
  _Float16* X16 = nullptr;           // fp16 passes (resnmtf_options.x_half, k <= 16): K-packed 2-byte image, tile stride (halves)
  size_t ld16 = 0, x16_halves = 0;
  // sparse view: the compressed copy it walks (SIDE_F: CSR, SIDE_G: CSC) and its work blocks: first line of each + end,
  // then a form flag per block
  long long* sp_ptr = nullptr;
  int* sp_idx = nullptr;
  float* sp_val = nullptr;
  int* sp_blk = nullptr;
  int sp_nblk = 0;
};

struct ViewState {
  int n = 0, m = 0, k = 0, KP = 16, NT = 1;
  int n_pad = 0, m_pad = 0;          // (= side[SIDE_F].pad, side[SIDE_G].pad)
  bool owned = true, has_x = false, has_factors = false;
  int empty_rows = 0, empty_cols = 0;          // all-zero rows / columns of the latest device-drawn data (shuffle, sub-sample)
  std::vector<unsigned char> empty_mask;     // [n + m], 1 = the row / column sums to zero
  unsigned char* ref_cl = nullptr;           // resnmtf_set_reference_clusters: [n][ref_k] row, then [m][ref_k] column clusters (0 / 1)
  int ref_k = 0;
  Side side[2];
  // fp16 passes (resnmtf_options.x_half, k <= 16): scale of the 2-byte images
  bool half = false, u16 = false;   // u16: uniform 16-bit integers instead of fp16 (x_half = 2, 3)
  bool half_capable = false;        // the 2-byte images are allocated; `half` says whether the passes use them (x_half = 3: guard)
  double x_relerr = 0.0;            // || X~ - X ||_F / || X ||_F of the 2-byte image (set at upload)
  float xscale = 1.f;
  double* xnorm2 = nullptr;
  double* S = nullptr;
  float* T32 = nullptr;              // (G side only: the f32 copy of T = X^T F the X.G launch's aux tiles read)
  int* fuse_cnt = nullptr;           // [2] arrivals of the update blocks fused into the Xt.F ([0]) / X.G ([1]) launch (pass_fused_kernel)
  double* sblk = nullptr;            // replicate_gs: the S update's inputs (sblock_layout), arena slice
  int kk_mode = 0;                   // 0 = A: Gram partials from the update kernels, k x k job = workgroup 0
                                     // 1 = B: Gram/cross/colsum on MFMA aux tiles, k x k job = last-arriving aux workgroup
  double *FtF = nullptr, *FtFS = nullptr, *cF = nullptr;
  KKFArgs argKF{};
  KKSArgs argKS{};
  // sparse view (resnmtf_create_sparse): CSC + CSR copies instead of the dense images, hand-off mode A, the passes are
  // spmm_kernel launches (resnmtf_sparse.hip.inc); the sides' nsplit are set at upload (<= kSparseMaxSplit[s])
  bool sparse = false;
  long long nnz_cap = 0, nnz = 0;
};

}  // namespace

struct resnmtf_handle {
  int V = 0;
  std::vector<ViewState> views;
  resnmtf_options opt{};
  hipStream_t stream = nullptr;       // every kernel of the loop (+ the host's exchanges)
  bool own_stream = false;
  std::vector<double> phi, xi, psi;   // V x V column-major
  SweepCtl* ctl = nullptr;
  double* err = nullptr;              // [err_cap][V]
  int err_cap = 0;
  int last_owned = -1;
  bool prepared = false;
  bool all_owned = true;
  // graphs
  // ladder of captured sweep graphs: check_every sweeps plus every smaller power of two, so that any run length
  // is a handful of graph launches (R/main.r:83-108 is the loop being replayed)
  std::vector<std::pair<int, hipGraphExec_t>> ladder;      // (sweeps, executable), descending
  std::vector<std::pair<int, hipGraphExec_t>> exact;       // short runs (< 3 batches) repeated with the same length: one graph each
  double graph_tol = -2.0;
  bool resume_ok = false;             // the device state is exactly what the run prologue would produce: skip it
  bool ctl_clean = false;             // ... and the loop control needs no reset either (fixed sweeps after fixed sweeps):
  int sweep_base = 0;                 //     the device's sweep counter then simply runs on: value at the START of the
  int next_base = 0;                  //     latest run / at its end
  SweepCtl* ctl_host = nullptr;       // pinned, device-mapped mirrors written by the k x k job of a sweep's last view /
  double* err_host = nullptr;         //   every view (fixed-iteration runs end with one stream synchronisation, no copy)
  SweepCtl* ctl_host_dev = nullptr;
  double* err_host_dev = nullptr;
  int n_cu = 256;                     // compute units of the device (multiProcessorCount)
  ChainArgs<8> chain[2]{};            // k <= 16: the F ([0], RESNMTF_PHASE_F_ALL) / G ([1], PHASE_G_ALL, replicated G chain) updates of
  int chain_views[2] = {0, 0};        //   every view in one launch (when eligible); 0 views = not eligible: one launch per view
  int chain_blocks[2] = {0, 0};
  WideChainArgs<8> wchain[2]{};       // k = 32 / 64: the F ([0]) and G ([1]) updates of every view in one launch (wide_chain_kernel)
  bool wchain_ok[2] = {false, false};
  int wchain_grid[2] = {0, 0};
  void* arena[2] = {nullptr, nullptr};          // replicate_f ([0]) / replicate_gs ([1]): the exchange blocks of all views, in view order
  size_t arena_bytes[2] = {0, 0};
  double* sblk_arena = nullptr; size_t sblk_stride = 0;        //   (S blocks: sblk_stride doubles each)
  bool sblk_embedded = false;         // the S block of a view sits at the end of its F block (equal-shaped views): they travel together
  double* sblk_base = nullptr; size_t sblk_step = 0;           // S block of view v = sblk_base + v * sblk_step (doubles)
  int* view_sweep = nullptr;          // replicate_gs: [V] sweeps closed per view (s_chain_kernel) + [1] its arrival counter
  double phase_tol = -1.0;            // phase API: >= 0 = convergence mode (resnmtf_set_stop_tolerance)
  int* fuse_err = nullptr;            // pinned, device-mapped: set by a fused pass launch whose wait for its update blocks ran out
  int* fuse_err_dev = nullptr;
  // slice_chains: rank r walks the F (G) chain of every view on the row (column) slice r; exchange buffers of the four
  // all-to-alls of a sweep (V chunks each) and the two chain launches
  bool sliced = false;
  int sl_len[2] = {0, 0};             // rows / columns per slice (multiples of 32)
  char *p_send[2] = {nullptr, nullptr}, *p_recv[2] = {nullptr, nullptr};      // the products U ([0]) / T ([1]) of the passes
  size_t p_chunk[2] = {0, 0};         // bytes per chunk: [per_slice][KP] f32 (+ the fp64 tail Ma_G | Md_G for T)
  float *w_send[2] = {nullptr, nullptr}, *w_recv[2] = {nullptr, nullptr};      // the new F / G rows: [V][per_slice][KP] f32 each
  // slice_p2p: the exchange as peer stores + stream-ordered flags (no collective): every rank's receive buffers and flag words,
  // mapped through hipIpc (own rank: the local pointers); flags[e] counts the arrivals of exchange e (0 U + S blocks, 1 new F
  // rows, 2 T slices, 3 new G rows): V per sweep
  struct Peer { char* p_recv[2] = {nullptr, nullptr}; float* w_recv[2] = {nullptr, nullptr}; double* sblk = nullptr;
                char* arena[2] = {nullptr, nullptr};      // block_p2p: the replicated layouts' exchange arenas
                unsigned int* flags = nullptr; bool imported = false; void* opened[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; };
  std::vector<Peer> peers;
  unsigned int* p2p_flags = nullptr;
  bool p2p_ready = false, p2p_prepared = false;
  unsigned int probe_epoch = 0;       // resnmtf_p2p_selftest calls so far (its arrival counter is cumulative)
  bool block_p2p = false;             // slice_p2p without slice_chains: the exchange blocks of the replicated layouts by peer stores
  double* slice_nd = nullptr;         // sliced chains in two launches: num | den of every view on this rank's slice (slice_products_kernel)
  WideChainArgs<8> schain[2]{};       // SLICE_F ([0]) / SLICE_G ([1])
  int schain_grid[2] = {0, 0};
  double ktime_ms[RESNMTF_TIMED_KINDS] = {0, 0, 0, 0, 0, 0};     // time_kernels: per kind (resnmtf_kernel_timings)
  long long klaunch[RESNMTF_TIMED_KINDS] = {0, 0, 0, 0, 0, 0};
  // pass timing (eager mode)
  std::vector<hipEvent_t> ev;         // pairs
  std::vector<int> ev_kind;           // 0 = xg, 1 = xtf per pair
  size_t ev_used = 0;
  resnmtf_pass_timing timing{};
  std::string last_error;

  int fail(int code, const std::string& msg) {
    last_error = msg;
    return code;
  }
  int fail_hip(const char* what, hipError_t e) {
    last_error = std::string(what) + ": " + hipGetErrorString(e);
    return RESNMTF_ERR_HIP;
  }
};

#define HIP_TRY(h, expr)                                      \
  do {                                                        \
    hipError_t e_ = (expr);                                   \
    if (e_ != hipSuccess) return (h)->fail_hip(#expr, e_);    \
  } while (0)

namespace {

template <typename T>
hipError_t dev_alloc_zero(T** p, size_t count) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess) return e;
  return hipMemset(*p, 0, std::max<size_t>(count, 1) * sizeof(T));
}

// The owner of a call's transient device memory: what take() hands out is freed when the object goes out of scope, on
// every path out of the function.  One hipMalloc per take() and nothing kept between calls.  After a failed take() it
// holds that error (error()), returns nullptr and allocates nothing further, so a run of take() calls is checked once.
// hipFree synchronises the device: declare a Scratch where it dies after the last stream synchronisation of its function.
class Scratch {
 public:
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { for (void* p : taken_) (void)hipFree(p); }
  template <class T>
  T* take(size_t count) {
    void* p = nullptr;
    if (err_ == hipSuccess) err_ = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (err_ != hipSuccess) return nullptr;
    taken_.push_back(p);
    return static_cast<T*>(p);
  }
  hipError_t error() const { return err_; }
 private:
  std::vector<void*> taken_;
  hipError_t err_ = hipSuccess;
};

// time_kernels: a pair of events for one launch of the given kind (RESNMTF_TIMED_*), attached to the dispatch itself
bool take_events(resnmtf_handle* h, int kind, hipEvent_t* e0, hipEvent_t* e1) {
  if (!h->opt.time_kernels || h->ev_used + 2 > h->ev.size()) return false;
  *e0 = h->ev[h->ev_used]; *e1 = h->ev[h->ev_used + 1];
  h->ev_kind[h->ev_used / 2] = kind;
  h->ev_used += 2;
  return true;
}
// ---- the launch layer.  Every kernel of the loop goes out through launch(); WHICH instantiation of a kernel family that is,
// is answered by the family's select_*() below and by nothing else: the launchers, set_all_attrs() (dynamic LDS limits) and
// resnmtf_view_plan() all read that one answer.  timed_kind: RESNMTF_TIMED_* or -1 (never timed).  In timed mode the
// start/stop events are attached to the dispatch itself, so the elapsed time is the kernel's own begin->end, the same
// quantity rocprofv3 --kernel-trace reports.  A null kernel is a form the planner chose and no selector lists: a bug in
// this file, not a case to fall back from.
template <class... KArgs, class... Args>
void launch(resnmtf_handle* h, int timed_kind, void (*kern)(KArgs...), dim3 grid, dim3 block, size_t smem, Args&&... args) {
  if (!kern) { std::fprintf(stderr, "resnmtf: no kernel instantiation for the launch form chosen\n"); std::abort(); }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (timed_kind >= 0 && take_events(h, timed_kind, &e0, &e1))
    hipExtLaunchKernelGGL(kern, grid, block, smem, h->stream, e0, e1, 0, static_cast<KArgs>(args)...);
  else
    hipLaunchKernelGGL(kern, grid, block, smem, h->stream, static_cast<KArgs>(args)...);
}

// f(std::integral_constant<int, V>{}) for the V of the list that equals x (the last one when none does)
template <int V0, int... Vs, class F>
auto pick_int(int x, F&& f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
  else return x == V0 ? f(std::integral_constant<int, V0>{}) : pick_int<Vs...>(x, f);
}
template <class F>
auto pick_kp(int KP, F&& f) { return pick_int<16, 32, 48, 64>(KP, f); }
// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <class F>
auto pick_bools(F&& f) { return f(); }
template <class F, class... Bs>
auto pick_bools(F&& f, bool b, Bs... bs) {
  return b ? pick_bools([&](auto... cs) { return f(std::true_type{}, cs...); }, bs...)
           : pick_bools([&](auto... cs) { return f(std::false_type{}, cs...); }, bs...);
}
constexpr int kKPs[] = {16, 32, 48, 64};
constexpr bool kBools[] = {false, true};

void free_view(ViewState& v) {
  for (Side& sd : v.side) {
    if (sd.xblk) { sd.xblk = nullptr; sd.xsum = nullptr; sd.Ma = nullptr; sd.Md = nullptr; sd.lm = nullptr; }   // arena slices
    void* ptrs[] = {sd.W, sd.W32, sd.Wk, sd.lm, sd.Ma, sd.Md, sd.part, sd.P, sd.Paux, sd.cnt, sd.X, sd.X16, sd.sp_ptr, sd.sp_idx, sd.sp_val, sd.sp_blk};
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
    for (auto& mp : sd.map)
      if (mp.dev) (void)hipFree(mp.dev);
  }
  v.sblk = nullptr;
  void* ptrs[] = {v.fuse_cnt, v.xnorm2, v.S, v.T32, v.FtF, v.FtFS, v.cF, v.ref_cl};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
}

int check_view(resnmtf_handle* h, int v) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (v < 0 || v >= h->V) return h->fail(RESNMTF_ERR_INVALID, "view index out of range");
  return RESNMTF_OK;
}

// column-major host -> row-major host
void to_row_major(const double* src, int rows, int cols, std::vector<double>& dst) {
  dst.resize((size_t)rows * cols);
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) dst[(size_t)i * cols + j] = src[(size_t)j * rows + i];
}
void to_col_major(const std::vector<double>& src, int rows, int cols, double* dst) {
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) dst[(size_t)j * rows + i] = src[(size_t)i * cols + j];
}

size_t update_smem_bytes(int KP) {
  const int UT = update_threads(KP), RG = UT / KP;      // (padded pitches of the fp64-MFMA form included)
  const int P16 = (KP % 32 == 0) ? KP + 16 : KP + 32;
  return sizeof(double) * ((size_t)2 * KP * P16 + 2 * (size_t)RG * (KP + 2) + (size_t)RG * KP + 2 * UT + 2 * (size_t)RG * P16);
}
size_t kk_smem_bytes(int KP, int NW) { return sizeof(double) * ((size_t)4 * KP * KP + 3 * 64 * (size_t)NW); }
size_t pass_smem_bytes(int KP, int NW) {
  const size_t tile_form = std::max(sizeof(float) * (size_t)std::max(NW / 2, 1) * 64 * KP, kk_smem_bytes(KP, NW));
  return KP > 16 ? std::max(tile_form, wide_smem_bytes(KP / 16)) : tile_form;
}
constexpr int kMaxLds = 160 * 1024;

// waves per workgroup: 8; k <= 16 also has 4- and 16-wave instantiations (tuning sweeps)
int max_pass_waves(int NT) { return NT <= 1 ? 16 : 8; }
// workgroups of a pass launch one CU holds at once: the kernels' __launch_bounds__ (kernels.hip.inc,
// pass_min_blocks) keeps the k <= 32 instantiations within 128 VGPRs
int pass_blocks_per_cu(int NT, int nw) { return pass_min_blocks(NT, nw); }

// ---- one selector per kernel family: run-time parameters -> the instantiation, as a typed function pointer
using PassFn = void (*)(PassArgs, KKFArgs, KKSArgs);
using FusedFn = void (*)(PassArgs, KKFArgs, KKSArgs, UpdateArgs, FuseArgs);
using SpmmFn = void (*)(SpmmArgs, KKFArgs, KKSArgs);
template <int NVB> using WideFn = void (*)(WideChainArgs<NVB>);

// pass_kernel at k <= 16 (NT = 1): exactly the forms of RESNMTF_PASS_K16_LIST, which is also what the second translation
// unit instantiates -- a form cannot be selectable without being emitted
struct PassK16Form { int nw, unroll; bool xg, mode_a; PassFn fn; };
const PassK16Form kPassK16[] = {
#define RESNMTF_FORM(NW, UNR, XG, MA) {NW, UNR, XG, MA, &pass_kernel<1, NW, UNR, XG, MA, 0>},
    RESNMTF_PASS_K16_LIST(RESNMTF_FORM)
#undef RESNMTF_FORM
};
// k > 16: 8 waves, UNROLL 4, and the only forms with a `wide` variant (SPLIT = 3: three bf16 pieces per operand)
PassFn select_pass(int NT, int nw, int unroll, bool xg, bool mode_a, bool wide) {
  if (NT <= 1) {
    for (const PassK16Form& f : kPassK16)
      if (!wide && f.nw == nw && f.unroll == unroll && f.xg == xg && f.mode_a == mode_a) return f.fn;
    return nullptr;
  }
  if (nw != 8 || unroll != 4) return nullptr;
  return pick_int<2, 3, 4>(NT, [&](auto nt) { return pick_bools([](auto x, auto m, auto w) {
    return &pass_kernel<decltype(nt)::value, 8, 4, decltype(x)::value, decltype(m)::value, (decltype(w)::value ? 3 : 0)>; }, xg, mode_a, wide); });
}
// pass_half_kernel (2-byte images: k <= 16, mode A, 8 waves).  No raised LDS limit: it asks for pass_smem_bytes(16, 8) = 20 KB
// plus pass_lds_pad_kb, which is within the 64 KB any kernel may have while pass_lds_pad_kb <= 44
PassFn select_pass_half(int unroll, bool xg, bool u16) {
  return pick_int<2, 3, 6, 4>(unroll, [&](auto un) { return pick_bools([](auto x, auto u) { return &pass_half_kernel<decltype(un)::value, decltype(x)::value, decltype(u)::value>; }, xg, u16); });
}
// pass_fused_kernel: UNROLL 4 = the ping-pong form, 8 the plain one; pre: with the prefetch of the first X trip
FusedFn select_pass_fused(int unroll, bool xg, bool pre) {
  return pick_int<4, 8>(unroll, [&](auto un) { return pick_bools([](auto x, auto p) { return &pass_fused_kernel<decltype(un)::value, decltype(x)::value, decltype(p)::value>; }, xg, pre); });
}
SpmmFn select_spmm(int KP, bool xg) {
  return pick_kp(KP, [&](auto kp) { return pick_bools([](auto x) { return &spmm_kernel<decltype(kp)::value, decltype(x)::value>; }, xg); });
}
// factor_update_kernel.  Coupling-count bucket of the instantiation: 0 = unrestricted form, else room for 4, 8 or 16 coupled views
constexpr int kCoupleBuckets[] = {0, 4, 8, RESNMTF_MAX_COUPLE};
int couple_bucket(const UpdateArgs& a) { return !a.restricted ? 0 : a.n_couple <= 4 ? 4 : a.n_couple <= 8 ? 8 : RESNMTF_MAX_COUPLE; }
auto select_update(int KP, bool g, int bucket, bool emit) {
  return pick_kp(KP, [&](auto kp) { return pick_int<0, 4, 8, RESNMTF_MAX_COUPLE>(bucket, [&](auto nc) {
    return pick_bools([](auto G, auto E) { return &factor_update_kernel<decltype(kp)::value, decltype(G)::value, decltype(nc)::value, decltype(E)::value>; }, g, emit);
  }); });
}
// f_chain_kernel<NVB, PF, IS_G>: the F form reads one folded slab per view (PF = 1) or up to four raw ones, the G form always one
template <int NVB>
auto select_f_chain(bool g, bool one_slab) { return g ? &f_chain_kernel<NVB, 1, true> : one_slab ? &f_chain_kernel<NVB, 1> : &f_chain_kernel<NVB, 4>; }
// wide_chain_kernel<KP, IS_G, NVB, SLICED>: the replicated chains exist for k > 16 only (build_wide_chain), the sliced ones at any k
template <int NVB>
WideFn<NVB> select_wide_chain(int KP, bool g, bool sliced) {
  return pick_kp(KP, [&](auto kp) { return pick_bools([](auto G, auto S) -> WideFn<NVB> {
    constexpr int K = decltype(kp)::value;
    if constexpr (decltype(S)::value) return &wide_chain_kernel<K, decltype(G)::value, NVB, true>;
    else if constexpr (K >= 32) return &wide_chain_kernel<K, decltype(G)::value, NVB>;
    else return nullptr;
  }, g, sliced); });
}
template <int NVB>
auto select_slice_chain(int KP, bool g) {
  return pick_kp(KP, [&](auto kp) { return pick_bools([](auto G) { return &slice_chain_kernel<decltype(kp)::value, decltype(G)::value, NVB>; }, g); });
}
// slice_products_kernel, slice_walk_kernel (4-row workgroups), slice_unpack_kernel: no dynamic LDS, so no raised limit
template <int NVB>
auto select_slice_products(int KP) { return pick_kp(KP, [](auto kp) { return &slice_products_kernel<decltype(kp)::value, NVB>; }); }
template <int NVB>
auto select_slice_walk(int KP) { return pick_kp(KP, [](auto kp) { return &slice_walk_kernel<decltype(kp)::value, NVB, 4>; }); }
auto select_slice_unpack(int KP) { return pick_kp(KP, [](auto kp) { return &slice_unpack_kernel<decltype(kp)::value>; }); }
// s_chain_kernel<KP, NVB>: room for 4, 8 or RESNMTF_MAX_COUPLE + 1 views
constexpr int kSChainViews[] = {4, 8, RESNMTF_MAX_COUPLE + 1};
auto select_s_chain(int KP, int n_views) {
  const int nvb = n_views <= 4 ? 4 : n_views <= 8 ? 8 : RESNMTF_MAX_COUPLE + 1;
  return pick_kp(KP, [&](auto kp) { return pick_int<4, 8, RESNMTF_MAX_COUPLE + 1>(nvb, [](auto nv) { return &s_chain_kernel<decltype(kp)::value, decltype(nv)::value>; }); });
}

// the dynamic LDS limit of every form the selectors can return, over their whole (finite) domains: what the launchers can
// select is attributed by construction.  The families without a raised limit say so at their selector.
hipError_t set_all_attrs() {
  hipError_t e = hipSuccess;
  auto lds = [&](auto* fn, size_t bytes) {      // (nullptr: a combination the family does not have)
    if (e == hipSuccess && fn) e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  };
  for (const PassK16Form& f : kPassK16) lds(f.fn, kMaxLds);
  for (bool xg : kBools)
    for (bool b : kBools) {
      for (int NT : {2, 3, 4}) { lds(select_pass(NT, 8, 4, xg, b, false), kMaxLds); lds(select_pass(NT, 8, 4, xg, b, true), kMaxLds); }
      for (int unroll : {4, 8}) lds(select_pass_fused(unroll, xg, b), kMaxLds);
    }
  for (int KP : kKPs) {
    for (bool g : kBools) {      // (g: IS_G of the updates and chains, IS_XG of spmm_kernel)
      for (int bucket : kCoupleBuckets) { lds(select_update(KP, g, bucket, false), update_smem_bytes(KP)); lds(select_update(KP, g, bucket, true), update_smem_bytes(KP)); }
      for (bool sliced : kBools) { lds(select_wide_chain<4>(KP, g, sliced), wide_chain_smem_bytes(KP)); lds(select_wide_chain<8>(KP, g, sliced), wide_chain_smem_bytes(KP)); }
      lds(select_slice_chain<4>(KP, g), slice_chain_smem_bytes(KP, 4)); lds(select_slice_chain<8>(KP, g), slice_chain_smem_bytes(KP, 8));
      lds(select_spmm(KP, g), kk_smem_bytes(KP, 8));
    }
    // (s_chain_kernel also holds a static table of NVB x NVB weights: static + dynamic must stay within the CU's LDS)
    for (int views : kSChainViews) lds(select_s_chain(KP, views), kMaxLds - 4096);
  }
  for (bool g : kBools)
    for (bool one_slab : kBools) { lds(select_f_chain<2>(g, one_slab), f_chain_smem_bytes<2>()); lds(select_f_chain<4>(g, one_slab), f_chain_smem_bytes<4>()); lds(select_f_chain<8>(g, one_slab), f_chain_smem_bytes<8>()); }
  return e;
}

// sparse view: X.G from the CSR, Xt.F from the CSC (spmm_kernel), same slabs as the dense passes.  kk: the k x k job in
// workgroup 0 (hand-off mode A, as pass_kernel); otherwise (SVD initialisation) B / P / width come from the caller
SpmmArgs spmm_args(const ViewState& v, bool xg) {
  const Side& sd = v.side[feeds(xg)];
  SpmmArgs a{};
  a.ptr = sd.sp_ptr; a.idx = sd.sp_idx; a.val = sd.sp_val; a.blk = sd.sp_blk; a.nblk = sd.sp_nblk; a.nsplit = sd.nsplit;
  a.B = v.side[other(feeds(xg))].W32; a.P = sd.P; a.cols_pad = sd.pad;
  a.ldb = v.KP;
  return a;
}
dim3 spmm_grid(const SpmmArgs& a) { return dim3((a.kk_block0 ? 1 : 0) + ceil_div(a.nblk * a.nsplit, 8)); }
size_t spmm_smem(const SpmmArgs& a, int KP) { return a.kk_block0 && !a.no_kk ? kk_smem_bytes(KP, 8) : 0; }
void launch_spmm(resnmtf_handle* h, const SpmmArgs& a, int KP, bool xg, const KKFArgs& kf, const KKSArgs& ks) {
  launch(h, -1, select_spmm(KP, xg), spmm_grid(a), dim3(512), spmm_smem(a, KP), a, kf, ks);
}

// ---- one streaming pass of a view, resolved: everything that is decided before the launch.  launch_pass launches from it,
// resnmtf_view_plan reports it, can_fuse_update and resnmtf_pass_timings read it
// aux products of a pass launch in hand-off mode B, by the side it feeds: X.G carries G^T G, T^T G, colSums(G); Xt.F F^T F, colSums(F)
constexpr int kAuxKinds[2] = {3, 2};
struct PassLaunch {
  int image = 0;               // what is streamed: 0 = f32 images, 1 = sparse CSC / CSR, 2 = fp16 image, 3 = 16-bit integer image
  bool mode_a = true;          // the k x k job is workgroup 0 (B: the last-arriving aux workgroup)
  bool fused = false;          // the update that feeds the pass rides in its first workgroups (pass_fused_kernel)
  bool wide = false;           // k > 16: three bf16 pieces per operand on the K = 32 MFMA, in wide workgroups
  bool xcd_order = false;      // XCD-aware order of the wide form's main workgroups (PassArgs::xcd_n)
  bool short_last = false;     // the last row split is shorter than the others
  bool pingpong = false;       // k <= 16, f32 images: the ping-pong prefetch form
  int waves = 8;
  int unroll = 0;              // pass_kernel / pass_fused_kernel UNROLL; pass_half_kernel: wave-steps per trip; sparse: 0
  int tiles_per_wg = 1;        // wide form: 64-column tiles per workgroup
  int lead_blocks = 1, main_blocks = 0;      // the k x k job / the aux workgroups head the grid
  dim3 grid, block;
  size_t smem = 0;
  PassFn kern = nullptr;       // exactly one of the three is set
  FusedFn kern_fused = nullptr;
  SpmmFn kern_spmm = nullptr;
};
// xg = false: Xt.F pass + kk_f;  xg = true: X.G pass + kk_s.  Reads the view's geometry (set at create / upload), not the
// argument blocks of resnmtf_prepare, so it answers before the first prepare as well
PassLaunch resolve_pass(const resnmtf_handle* h, const ViewState& v, bool xg, bool fuse_update = false) {
  PassLaunch L;
  if (v.sparse) {      // X.G from the CSR, Xt.F from the CSC (spmm_kernel), hand-off mode A at every k
    SpmmArgs a = spmm_args(v, xg);
    a.kk_block0 = 1;
    L.image = 1;
    L.main_blocks = ceil_div(a.nblk * a.nsplit, 8);
    L.grid = spmm_grid(a); L.block = dim3(512);
    L.smem = spmm_smem(a, v.KP);
    L.kern_spmm = select_spmm(v.KP, xg);
    return L;
  }
  const Side& sd = v.side[feeds(xg)];
  const int nw = sd.nw, nsplit = sd.nsplit, rps = sd.rps;
  const int rows_pad = v.side[other(feeds(xg))].pad, ntiles = sd.pad / 64;      // (the reduction runs over the OTHER side's lines)
  L.image = v.half ? (v.u16 ? 3 : 2) : 0;
  L.mode_a = v.kk_mode == 0;
  L.waves = nw;
  // MFMA form of the main tiles (resnmtf_options.bf16_split): k <= 16 always the f32 MFMA; k > 16: three bf16 pieces per
  // operand on the K = 32 MFMA in wide workgroups (f32-grade, default; 1 is accepted as an alias), 2 = plain f32 MFMA
  L.wide = v.NT >= 2 && h->opt.bf16_split != 2;
  L.xcd_order = L.wide && h->opt.xcd_order;
  L.short_last = nsplit > 1 && rows_pad - (nsplit - 1) * rps < rps;
  L.tiles_per_wg = L.wide ? sd.tw : 1;
  L.main_blocks = ceil_div(ntiles, L.tiles_per_wg) * nsplit;
  L.lead_blocks = L.mode_a ? 1 : kAuxKinds[feeds(xg)] * sd.nsaux;
  L.grid = dim3(L.lead_blocks + L.main_blocks); L.block = dim3(64 * nw);
  L.smem = std::min<size_t>(pass_smem_bytes(v.KP, nw) + (size_t)h->opt.pass_lds_pad_kb * 1024, kMaxLds);
  const bool pp = sd.pp;
  if (fuse_update) {
    L.fused = true;
    L.pingpong = pp;
    L.unroll = pp ? 4 : 8;
    L.smem = std::min<size_t>(std::max(L.smem, update_smem_bytes(16)), kMaxLds);
    L.kern_fused = select_pass_fused(L.unroll, xg, h->opt.fuse_updates == 1);   // (2: without the prefetch of the first X trip)
  } else if (v.half) {
    // wave-steps per trip: 4 for fp16; 2 for the 16-bit integers (their widening to f32 wants the registers: c2 26.5 k
    // sweeps/s at 2, 23.5 k at 4).  (pass_half_kernel has no ping-pong form)
    const int hu = h->opt.half_unroll;
    L.unroll = (hu == 2 || hu == 3 || hu == 4 || hu == 6) ? hu : (v.u16 ? 2 : 4);
    L.kern = select_pass_half(L.unroll, xg, v.u16);
  } else {
    L.pingpong = v.NT == 1 && nw == 8 && pp;
    L.unroll = v.NT >= 2 ? 4 : (nw == 8 ? (pp ? 4 : RESNMTF_K16_UNROLL) : 8);
    L.kern = select_pass(v.NT, nw, L.unroll, xg, L.mode_a, L.wide);
  }
  return L;
}
// can the F (kind 0) / G (kind 1) update of view v ride in the pass launch that consumes it (pass_fused_kernel)?  Mode A at
// k <= 16 with the f32 images and 8-wave workgroups, the unrestricted update form (the coupled forms exceed the pass's
// register budget), and few enough row blocks that every updater is resident among the launch's first workgroups
bool can_fuse_update(const resnmtf_handle* h, const ViewState& v, int kind) {
  if (h->opt.fuse_updates == 0 || v.NT != 1 || !v.fuse_cnt) return false;
  const PassLaunch L = resolve_pass(h, v, kind != 0);
  if (L.image != 0 || !L.mode_a || L.waves != 8) return false;
  const Side& sd = v.side[kind];
  return !sd.arg.restricted && sd.nblk <= L.main_blocks && sd.nblk <= h->n_cu;
}
// (The k x k job's dynamic LDS is requested for every workgroup of the launch: at KP >= 48 one workgroup per CU.  Measured,
// 200000 x 20000 at 0.5 %, k = 64: the Xt.F pass alone runs 632-650 us without that LDS against 846 us with it, but the job
// as a launch of its own then takes 354 us behind it (the fp64 partials of 512 update workgroups) -- 1004 us in all -- so it
// stays in workgroup 0, where it overlaps the pass.  DESIGN.md section 10.)
// kk_s mode: 0 = run prologue, 1 = full S update
void launch_pass(resnmtf_handle* h, const ViewState& v, bool xg, int mode, double tol, bool check_done, bool fuse_update = false) {
  const PassLaunch L = resolve_pass(h, v, xg, fuse_update);
  const int kind = xg ? RESNMTF_TIMED_XG : RESNMTF_TIMED_XTF;
  KKFArgs kf = v.argKF;
  KKSArgs ks = v.argKS;
  ks.mode = mode; ks.tol = tol;
  if (L.kern_spmm) {
    SpmmArgs a = spmm_args(v, xg);
    a.kk_block0 = 1; a.no_kk = 0; a.ctl = h->ctl; a.check_done = check_done ? 1 : 0;
    launch(h, kind, L.kern_spmm, L.grid, L.block, L.smem, a, kf, ks);
    return;
  }
  PassArgs a = v.side[feeds(xg)].pass;
  a.check_done = check_done ? 1 : 0;
  // mode A: the k x k job is workgroup 0 and reads the update kernel's fp64 partials
  a.kk_block0 = L.mode_a ? 1 : 0;
  a.fuse_zero = (a.kk_block0 && v.fuse_cnt && !v.half) ? v.fuse_cnt + (xg ? 0 : 2) : nullptr;   // the sibling launch's arrival counter
  if (!a.kk_block0) { kf.part = nullptr; ks.part = nullptr; }
  a.xcd_n = 0;
  if (L.xcd_order) {      // a short last split stays at the end of the grid
    const int n_map = L.short_last ? (a.nsplit - 1) * a.ntg : L.main_blocks;
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int x = 0; x < 8; ++x) a.xcd_first[x] = -1;
    for (int b = 0; b < n_map; ++b) {
      const int x = (L.lead_blocks + b) & 7;
      if (a.xcd_first[x] < 0) a.xcd_first[x] = L.lead_blocks + b;
      ++cnt[x];
    }
    int off = 0;
    for (int x = 0; x < 8; ++x) { a.xcd_off[x] = off; off += cnt[x]; if (a.xcd_first[x] < 0) a.xcd_first[x] = 0; }
    a.xcd_n = n_map;
  }
  if (L.fused) {
    const Side& upd = v.side[other(feeds(xg))];      // the update of the pass's B operand
    UpdateArgs u = upd.arg;
    u.check_done = 0; u.gram_only = 0;
    FuseArgs fz{};
    fz.cnt_own = v.fuse_cnt + (xg ? 2 : 0);      // [0] arrivals, [1] the flag the waiters poll
    { static const int nap = std::getenv("RESNMTF_FUSE_NAP") ? std::atoi(std::getenv("RESNMTF_FUSE_NAP")) : 2; fz.nap = nap; }
    fz.n_upd = upd.nblk; fz.err = h->fuse_err_dev;
    launch(h, kind, L.kern_fused, L.grid, L.block, L.smem, a, kf, ks, u, fz);
    return;
  }
  // 2-byte image of X: the run-time scale (set at upload) is taken out in the slab store
  if (L.image >= 2) a.out_scale = v.u16 ? 1.f / v.xscale : 1.f / (v.xscale * RESNMTF_B16_SCALE);
  launch(h, kind, L.kern, L.grid, L.block, L.smem, a, kf, ks);
}

// a streaming pass without a k x k job (SVD initialisation): the default mode A form of the view's k, workgroup 0 idles
void launch_pass_plain(resnmtf_handle* h, PassArgs a, int NT, bool xg) {
  a.kk_block0 = 1; a.no_kk = 1; a.check_done = 0;
  const dim3 grid(1 + a.ntiles * a.nsplit), block(64 * 8);
  const size_t smem = std::min<size_t>(pass_smem_bytes(16 * NT, 8), kMaxLds);
  launch(h, -1, select_pass(NT, 8, NT <= 1 ? RESNMTF_K16_UNROLL : 4, xg, true, false), grid, block, smem, a, KKFArgs{}, KKSArgs{});
}

template <int NVB>
ChainArgs<NVB> narrow_chain(const ChainArgs<8>& c) {
  ChainArgs<NVB> a{};
  a.len = c.len; a.k = c.k; a.n_views = c.n_views; a.rows_per_block = c.rows_per_block;
  a.n_emit = c.n_emit; a.restricted = c.restricted; a.ctl = c.ctl; a.check_done = c.check_done; a.pstride = c.pstride;
  a.kpack32 = c.kpack32;
  for (int e = 0; e < 4; ++e) { a.W32e[e] = c.W32e[e]; a.parte[e] = c.parte[e]; a.T32e[e] = c.T32e[e]; }
  for (int v = 0; v < NVB; ++v) {
    a.emit_slot[v] = c.emit_slot[v];
    a.W[v] = c.W[v]; a.U[v] = c.U[v]; a.nsplit[v] = c.nsplit[v]; a.Ma[v] = c.Ma[v]; a.Md[v] = c.Md[v]; a.lm[v] = c.lm[v];
    a.sigma[v] = c.sigma[v]; a.n_other[v] = c.n_other[v]; a.cmask[v] = c.cmask[v];
    for (int w = 0; w < NVB; ++w) a.weight[v][w] = c.weight[v][w];
  }
  return a;
}

// kind: 0 = F update, 1 = G update, 2 = mode A run prologue: partials of the current G, nothing updated
void launch_update(resnmtf_handle* h, const ViewState& v, int kind, bool check_done) {
  const Side& sd = v.side[kind == 0 ? SIDE_F : SIDE_G];
  UpdateArgs a = sd.arg;
  a.check_done = check_done ? 1 : 0;
  a.gram_only = kind == 2 ? 1 : 0;
  if (kind == 2) { a.restricted = 0; a.n_couple = 0; }
  launch(h, -1, select_update(v.KP, kind != 0, couple_bucket(a), v.kk_mode == 0), dim3(sd.nblk), dim3(update_threads(v.KP)), update_smem_bytes(v.KP), a);
}

template <int NVB>
WideChainArgs<NVB> narrow_wchain(const WideChainArgs<8>& c) {
  WideChainArgs<NVB> a{};
  a.len = c.len; a.k = c.k; a.n_views = c.n_views; a.ngroups = c.ngroups; a.own = c.own; a.n_self = c.n_self; a.O32 = c.O32; a.o32_stride = c.o32_stride;
  a.W32 = c.W32; a.Wk = c.Wk; a.T32 = c.T32; a.ld32 = c.ld32; a.ctl = c.ctl; a.check_done = c.check_done; a.restricted = c.restricted;
  for (int v = 0; v < NVB; ++v) {
    a.W[v] = c.W[v]; a.U[v] = c.U[v]; a.Ma[v] = c.Ma[v]; a.Md[v] = c.Md[v]; a.lm[v] = c.lm[v]; a.O32v[v] = c.O32v[v];
    a.sigma[v] = c.sigma[v]; a.n_other[v] = c.n_other[v]; a.cmask[v] = c.cmask[v];
    for (int w = 0; w < NVB; ++w) a.weight[v][w] = c.weight[v][w];
  }
  return a;
}
// the chain kernels are instantiated for 4 or 8 views (f_chain_kernel: 2, 4 or 8): f(width, the arguments narrowed to it)
template <class F>
void for_wchain(const WideChainArgs<8>& c, F&& f) {
  if (c.n_views <= 4) f(std::integral_constant<int, 4>{}, narrow_wchain<4>(c));
  else f(std::integral_constant<int, 8>{}, c);
}
template <class F>
void for_chain(const ChainArgs<8>& c, int views, F&& f) {
  if (views <= 2) f(std::integral_constant<int, 2>{}, narrow_chain<2>(c));
  else if (views <= 4) f(std::integral_constant<int, 4>{}, narrow_chain<4>(c));
  else f(std::integral_constant<int, 8>{}, c);
}
// update_f (g == 0) or update_g (g == 1) of every view in one launch (wide_chain_kernel): the replicated chains (all rows,
// k > 16) or -- sliced -- this rank's row / column slice of them (any k)
void launch_wide_chain(resnmtf_handle* h, int g, bool checked, bool sliced = false) {
  WideChainArgs<8>& c = sliced ? h->schain[g] : h->wchain[g];
  c.check_done = checked ? 1 : 0;
  const int KP = h->views[0].KP;
  const size_t smem = wide_chain_smem_bytes(KP);
  const int ngrid = sliced ? h->schain_grid[g] : h->wchain_grid[g];
  if (ngrid < 1) return;                                   // (an empty slice)
  const int kind = g == 0 ? RESNMTF_TIMED_F_CHAIN : RESNMTF_TIMED_G_CHAIN;
  // sliced: the products-first kernel on 16-row groups (slice_chain_kernel); RESNMTF_SLICE_WIDE=1 keeps the view-by-view
  // walk of wide_chain_kernel on 32-row groups (A/B testing -- same bits either way)
  // Which of the two: a slice_chain workgroup finishes one 16-row group in ~35 us at k = 64 (latency: 4 product stages + 8
  // walk steps), a wide_chain workgroup a 32-row group in ~50 us -- so the 16-row form wins while its groups fit ONE round
  // of resident workgroups (c5 x 8: the G slices, 64 groups; c4 x 4: both chains) and loses when they need two (c5 x 8, F:
  // 392 groups on 256 CUs, 70 against 53 us).  RESNMTF_SLICE_WIDE=1 / =0 forces one form (A/B testing).
  static const char* slice_env = std::getenv("RESNMTF_SLICE_WIDE");
  const int groups16_all = ceil_div(c.len, 16);
  const int n_slots = h->n_cu * (int)std::max<size_t>(1, std::min<size_t>(kMaxLds / slice_chain_smem_bytes(KP, c.n_views <= 4 ? 4 : 8), 2048 / (16 * KP)));
  const bool slice_wide = slice_env ? slice_env[0] == '1' : groups16_all > n_slots;
  // ... and the 16-row form itself in two launches (slice_products_kernel: every (group, pair of views) a workgroup of its own;
  // slice_walk_kernel: the element-wise chain), unless RESNMTF_SLICE_FUSED=1 keeps it in one (slice_chain_kernel) -- same bits
  // Measured (tools/round3/slice_split_ab.sh): c5 x 8, G slice (8 views, k = 64, 63 groups) 36.0 -> 22.4 us; c4 x 4 (4 views,
  // k = 32: two short product stages) 11.2 -> 15.2 / 9.4 -> 10.5 us -- the second launch costs more than the stages it spreads.
  // So: more than two pairs of views and k > 32; RESNMTF_SLICE_FUSED=1 / =0 forces one form.
  static const char* fused_env = std::getenv("RESNMTF_SLICE_FUSED");
  const bool split_form = fused_env ? fused_env[0] == '0' : (c.n_views > 4 && KP > 32);
  if (sliced && !slice_wide && h->slice_nd && split_form) {
    const int groups16 = ceil_div(c.len, 16);
    const unsigned nd_stride = (unsigned)groups16 * 16u * (unsigned)KP;
    const dim3 gridp(groups16, (c.n_views + 1) / 2), gridw(ceil_div(c.len, 4)), block16(16 * KP), blockw(4 * KP);
    for_wchain(c, [&](auto nvb, const auto& a) {
      constexpr int NVB = decltype(nvb)::value;
      launch(h, kind, select_slice_products<NVB>(KP), gridp, block16, 0, a, h->slice_nd, nd_stride);
      launch(h, kind, select_slice_walk<NVB>(KP), gridw, blockw, 0, a, h->slice_nd, nd_stride);
    });
    return;
  }
  if (sliced && !slice_wide) {
    const dim3 grid16(ceil_div(c.len, 16)), block16(16 * KP);          // (one row group per workgroup)
    for_wchain(c, [&](auto nvb, const auto& a) {
      constexpr int NVB = decltype(nvb)::value;
      launch(h, kind, select_slice_chain<NVB>(KP, g != 0), grid16, block16, slice_chain_smem_bytes(KP, NVB), a);
    });
    return;
  }
  const dim3 grid(ngrid), block(16 * KP);
  for_wchain(c, [&](auto nvb, const auto& a) {
    launch(h, kind, select_wide_chain<decltype(nvb)::value>(KP, g != 0, sliced), grid, block, smem, a);
  });
}

// the F updates of every view as ONE f_chain_kernel launch: is the chain there (enqueue_phase_f_all launches it), does
// resnmtf_run's sweep hoist it ahead of the views (F_w' reads neither G nor S of the same sweep; every view owned), its
// view-count instantiation, and does it read one X.G slab per view?
struct FChainPlan { bool chain = false, hoisted = false, one_slab = true; int width = 0; };
FChainPlan plan_f_chain(const resnmtf_handle* h) {
  FChainPlan p;
  p.chain = !h->wchain_ok[0] && h->chain_views[SIDE_F] > 0;
  if (!p.chain) return p;
  p.hoisted = h->all_owned;
  p.width = h->chain_views[SIDE_F] <= 2 ? 2 : (h->chain_views[SIDE_F] <= 4 ? 4 : 8);
  for (int v = 0; v < h->chain_views[SIDE_F]; ++v) p.one_slab = p.one_slab && h->chain[SIDE_F].nsplit[v] == 1;
  return p;
}
// the k <= 16 chain of side s (every view's update of that side) as ONE f_chain_kernel launch; false: not eligible
bool enqueue_chain(resnmtf_handle* h, int s, bool one_slab, bool checked) {
  if (h->chain_views[s] <= 0) return false;
  h->chain[s].check_done = checked ? 1 : 0;
  const int kind = s == SIDE_F ? RESNMTF_TIMED_F_CHAIN : RESNMTF_TIMED_G_CHAIN;
  for_chain(h->chain[s], h->chain_views[s], [&](auto nvb, const auto& a) {
    constexpr int NVB = decltype(nvb)::value;
    launch(h, kind, select_f_chain<NVB>(s == SIDE_G, one_slab), dim3(h->chain_blocks[s]), dim3(512), f_chain_smem_bytes<NVB>(), a);
  });
  return true;
}
// RESNMTF_PHASE_F_ALL: update_f of every view in view order (one launch when the chain is eligible)
void enqueue_phase_f_all(resnmtf_handle* h, bool checked = false) {
  if (h->wchain_ok[0]) { launch_wide_chain(h, 0, checked); return; }
  const FChainPlan p = plan_f_chain(h);
  if (p.chain && enqueue_chain(h, SIDE_F, p.one_slab, checked)) return;
  for (const auto& v : h->views)
    if (v.owned || v.side[SIDE_F].replica) launch_update(h, v, 0, checked);
}

// ---- the phases of one view (see the header comment)
void enqueue_phase_f(resnmtf_handle* h, const ViewState& v, bool checked) { launch_update(h, v, 0, checked); }
// replicate_f / replicate_gs: the split slabs of the pass that feeds side s of an owned view -> the one f32 slab of its
// exchange block (what every rank's update of this view reads, the owner's included: a third of the bytes on the wire at c2)
void launch_fold(resnmtf_handle* h, const ViewState& v, int s) {
  const Side& sd = v.side[s];
  if (!sd.xsum) return;
  const int quads = sd.pad * v.KP / 4;
  launch(h, RESNMTF_TIMED_PACK, slab_fold_kernel, dim3(ceil_div(quads, 256)), dim3(256), 0, sd.P, sd.nsplit, quads, sd.xsum);
}
// slice_chains: the own view's pass result, folded and cut into the V chunks of the next all-to-all (slice_pack_kernel)
void launch_slice_pack(resnmtf_handle* h, const ViewState& v, bool xg, bool checked) {
  SlicePackArgs a{};
  const int s = feeds(xg);
  const Side& sd = v.side[s];
  a.P = sd.P; a.nsplit = sd.nsplit; a.rows_pad = sd.pad;
  a.KP = v.KP; a.NT = v.NT;
  a.rows_per_slice = h->sl_len[s]; a.n_slices = h->opt.slice_count;
  a.out = h->p_send[s]; a.chunk_bytes = h->p_chunk[s];
  if (!xg) { a.tail[0] = sd.Ma; a.tail[1] = sd.Md; a.tail_count = v.k * v.k; a.T32 = v.T32; a.ld32 = 64; }
  if (h->opt.slice_p2p) {      // chunk c straight into rank c's receive slot for this rank; U: the own S block into every rank's arena
    const int r = h->opt.slice_index, vi = (int)(&v - h->views.data());
    a.out = nullptr;
    for (int c = 0; c < a.n_slices; ++c) {
      const resnmtf_handle::Peer& pc = h->peers[(size_t)c];
      a.outv[c] = pc.p_recv[s] + (size_t)r * a.chunk_bytes;
      if (xg) a.tailv[c] = pc.sblk + (size_t)vi * h->sblk_stride;
    }
    if (xg) { a.tail[0] = v.sblk; a.tail[1] = v.sblk + h->sblk_stride / 2; a.tail_count = (int)(h->sblk_stride / 2); }
  }
  a.ctl = h->ctl; a.check_done = checked ? 1 : 0;
  const size_t quads = (size_t)a.n_slices * a.rows_per_slice * (a.KP / 4);
  launch(h, RESNMTF_TIMED_PACK, slice_pack_kernel, dim3((unsigned)std::min<size_t>((quads + 255) / 256, 65535)), dim3(256), 0, a);
}
// slice_p2p: one arrival on every rank's counter of exchange e (stream-ordered behind the kernels that stored the data) /
// the stream waits until `arrivals` of them are in
void p2p_signal(resnmtf_handle* h, int e) {
  SliceSignalArgs a{};
  a.n = h->V;
  for (int c = 0; c < h->V; ++c) a.flag[c] = h->peers[(size_t)c].flags + e;
  hipLaunchKernelGGL(slice_signal_kernel, dim3(1), dim3(64), 0, h->stream, a);
}
// the stream goes on when counter e has V * (waits of this call site so far + add) arrivals.  slice_p2p = 1: the command
// processor waits (hipStreamWaitValue32; the host's sweep index numbers the wait); 2: p2p_wait_kernel (site counters on the device)
hipError_t p2p_wait(resnmtf_handle* h, int e, int site, int sweep, int add) {
  if (h->opt.slice_p2p != 2)
    return hipStreamWaitValue32(h->stream, h->p2p_flags + e, (unsigned)h->V * (unsigned)(sweep + add), hipStreamWaitValueGte, 0xFFFFFFFFu);
  P2pWaitArgs a{};
  a.flag = h->p2p_flags + e; a.site = h->p2p_flags + 16 + site; a.per_wait = (unsigned)h->V; a.add = (unsigned)add; a.err = h->fuse_err_dev;
  hipLaunchKernelGGL(p2p_wait_kernel, dim3(1), dim3(64), 0, h->stream, a);
  return hipGetLastError();
}
// block_p2p: byte ranges [off0, off0 + b0) and [off1, off1 + b1) of this rank's part of an arena -> the same place on every peer
// kind SIDE_F / SIDE_G: that exchange arena, 2: S block arena
void launch_block_push(resnmtf_handle* h, int kind, size_t off0, size_t b0, size_t off1, size_t b1) {
  BlockPushArgs a{};
  a.src = static_cast<const char*>(kind < 2 ? h->arena[kind] : (void*)h->sblk_arena);
  for (int c = 0; c < h->V; ++c) {
    if (c == h->opt.slice_index) continue;
    const resnmtf_handle::Peer& pc = h->peers[(size_t)c];
    a.dst[a.n_dst++] = kind < 2 ? pc.arena[kind] : reinterpret_cast<char*>(pc.sblk);
  }
  if (a.n_dst == 0) return;
  a.off[0] = off0; a.bytes[0] = b0; a.off[1] = off1; a.bytes[1] = b1;
  const size_t quads = (b0 + b1) / 16;
  launch(h, RESNMTF_TIMED_PACK, block_push_kernel, dim3((unsigned)std::max<size_t>(1, std::min<size_t>((quads + 255) / 256, 2048))), dim3(256), 0, a);
}
// the exchange block of side s of an owned view to the peers.  F: everything (replicate_f alone: the owner's coefficients and
// lambda are the only copy) or, with the replicated S chain, the U rows and the S block only -- every rank computes the
// coefficients, lambda and mu of every view itself and a late store must not land on them.  G: [Tsum | Ma_G | Md_G], not mu
void push_block(resnmtf_handle* h, const ViewState& v, int s) {
  const Side& sd = v.side[s];
  const size_t base = (size_t)(static_cast<const char*>(sd.xblk) - static_cast<const char*>(h->arena[s]));
  const size_t sum = ((size_t)sd.pad * v.KP * sizeof(float) + 255) / 256 * 256;
  if (s == SIDE_G) { launch_block_push(h, s, base, (sum + 2 * (size_t)v.k * v.k * sizeof(double)) / 16 * 16, 0, 0); return; }
  if (!h->opt.replicate_gs) { launch_block_push(h, s, base, sd.xblk_bytes, 0, 0); return; }
  if (h->sblk_embedded) {      // the S block travels with the U rows: the F-side special case
    const size_t s_off = (size_t)(reinterpret_cast<const char*>(v.sblk) - static_cast<const char*>(h->arena[s]));
    launch_block_push(h, s, base, sum, s_off, h->sblk_stride * sizeof(double));
  } else {
    launch_block_push(h, s, base, sum, 0, 0);
    const size_t sb = (h->sblk_stride * sizeof(double));
    launch_block_push(h, 2, (size_t)(&v - h->views.data()) * sb, sb / 16 * 16, 0, 0);
  }
}
// slice_chains: the own view's new F (g == 0) / G (g == 1) rows, as received, -> the operand copies of the next pass
void launch_slice_unpack(resnmtf_handle* h, const ViewState& v, int g, bool checked) {
  SliceUnpackArgs a{};
  a.in = h->w_recv[g]; a.len = v.side[g].len; a.k = v.k;
  a.W32 = v.side[g].W32; a.ld32 = 64; a.Wk = v.side[g].Wk;
  a.ctl = h->ctl; a.check_done = checked ? 1 : 0;
  launch(h, RESNMTF_TIMED_PACK, select_slice_unpack(v.KP), dim3(ceil_div(a.len, 32)), dim3(256), 0, a);
}
// replicate_gs: the second half of the k x k job of EVERY view (update_s chain, update_lm, error, F coefficients)
int launch_s_chain(resnmtf_handle* h, bool checked) {
  SChainArgs a{};
  const int V = h->V;
  const ViewState& v0 = h->views[0];
  a.k = v0.k; a.n_views = V;
  a.view_sweep = h->view_sweep; a.ticket = h->view_sweep + V;
  a.tol = h->phase_tol; a.check_done = checked ? 1 : 0;
  a.sblocks = h->sblk_base; a.sblock_stride = h->sblk_step;
  double sum_xi = 0.0;
  for (double x : h->xi) sum_xi += x;
  a.restricted = sum_xi != 0.0 ? 1 : 0;
  for (int w = 0; w < V; ++w) {
    const ViewState& vs = h->views[w];
    a.S[w] = vs.S; a.lambda[w] = vs.side[SIDE_F].lm; a.mu[w] = vs.side[SIDE_G].lm; a.Ma_F[w] = vs.side[SIDE_F].Ma; a.Md_F[w] = vs.side[SIDE_F].Md;
    double sg = 0.0;
    for (int c = 0; c < V; ++c) {
      const double wgt = h->xi[(size_t)c + (size_t)w * V];                          // xi[c, w]
      a.xi[c][w] = (c == w) ? 0.0 : wgt;
      sg += wgt;
    }
    a.sigma[w] = sg;
  }
  a.err = h->err; a.err_stride = V; a.err_cap = h->err_cap; a.err_host = h->err_host_dev;
  a.ctl = h->ctl; a.ctl_host = h->ctl_host_dev;
  const size_t smem = kk_smem_bytes(v0.KP, 16);
  launch(h, RESNMTF_TIMED_S_CHAIN, select_s_chain(v0.KP, V), dim3(V), dim3(s_chain_threads(v0.KP)), smem, a);
  return RESNMTF_OK;
}
// fuse_f: the view's F update has NOT been enqueued -- it rides in the Xt.F launch (enqueue_sweep decides)
void enqueue_phase_g(resnmtf_handle* h, const ViewState& v, double tol, bool checked, bool fuse_f = false) {
  launch_pass(h, v, false, 1, tol, checked, fuse_f);
  const bool fuse_g = can_fuse_update(h, v, 1);
  if (!fuse_g) launch_update(h, v, 1, checked);
  launch_pass(h, v, true, 1, tol, checked, fuse_g);
  launch_fold(h, v, SIDE_F);
}
// run prologue of one view: X.G launch whose kk_s runs in mode 0 (F coefficients from the current S, G);
// mode A first emits the fp64 partials of the current G so that a resumed run is bitwise identical
void enqueue_prologue(resnmtf_handle* h, const ViewState& v) {
  if (v.kk_mode == 0) launch_update(h, v, 2, false);
  launch_pass(h, v, true, 0, -1.0, false);
  launch_fold(h, v, SIDE_F);
  if (h->sliced) launch_slice_pack(h, v, true, false);
  if (h->sliced && h->opt.slice_p2p) p2p_signal(h, 0);
}

void enqueue_sweep(resnmtf_handle* h, double tol) {
  const bool checked = tol >= 0.0;
  // F_w' reads neither G nor S of the same sweep: when the fused chain applies (several k <= 16 views sharing
  // their rows in the same order) every F update of the sweep runs first, in one launch
  const bool hoist = plan_f_chain(h).hoisted;
  if (hoist) enqueue_phase_f_all(h, checked);
  for (const auto& v : h->views) {
    if (!v.owned) continue;
    const bool fuse_f = !hoist && can_fuse_update(h, v, 0);
    if (!hoist && !fuse_f) enqueue_phase_f(h, v, checked);
    enqueue_phase_g(h, v, tol, checked, fuse_f);
  }
}

void destroy_graphs(resnmtf_handle* h) {
  for (auto& rung : h->ladder)
    if (rung.second) (void)hipGraphExecDestroy(rung.second);
  h->ladder.clear();
  for (auto& g : h->exact)
    if (g.second) (void)hipGraphExecDestroy(g.second);
  h->exact.clear();
  h->graph_tol = -2.0;
}

int capture_graph(resnmtf_handle* h, int sweeps, double tol, hipGraphExec_t* out) {
  hipGraph_t g = nullptr;
  HIP_TRY(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  for (int s = 0; s < sweeps; ++s) enqueue_sweep(h, tol);
  HIP_TRY(h, hipStreamEndCapture(h->stream, &g));
  hipError_t e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return h->fail_hip("hipGraphInstantiate", e);
  (void)hipGraphUpload(*out, h->stream);      // first replay does not pay the upload
  return RESNMTF_OK;
}
// the whole ladder at once (a few hundred kernel nodes): a later run of any length never captures inside a timed region
int capture_ladder(resnmtf_handle* h, int batch, double tol) {
  for (auto& rung : h->ladder)
    if (rung.second) (void)hipGraphExecDestroy(rung.second);
  h->ladder.clear();
  std::vector<int> rungs{batch};
  int p2 = 1;
  while (p2 * 2 < batch) p2 *= 2;
  for (; p2 >= 1; p2 /= 2)
    if (p2 < batch) rungs.push_back(p2);
  for (int sweeps : rungs) {
    hipGraphExec_t ex = nullptr;
    if (int rc = capture_graph(h, sweeps, tol, &ex)) { destroy_graphs(h); return rc; }
    h->ladder.emplace_back(sweeps, ex);
  }
  return RESNMTF_OK;
}

// RESNMTF_PHASE_LOCAL_SWEEP: every F update this handle holds inputs for, then PHASE_G of every owned view
void enqueue_local_sweep(resnmtf_handle* h) {
  enqueue_phase_f_all(h);
  for (const auto& v : h->views)
    if (v.owned) enqueue_phase_g(h, v, -1.0, false);
}
// (Replaying these five launches from a hipGraph between two RCCL collectives was measured SLOWER than the plain
// launches: 61.8 against 54.8 us per sweep with one rank -- a graph launch per sweep costs more than it saves.)
int launch_local_sweep(resnmtf_handle* h) {
  enqueue_local_sweep(h);
  return RESNMTF_OK;
}

int flush_timing(resnmtf_handle* h) {
  if (h->ev_used == 0) return RESNMTF_OK;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
    const int kind = h->ev_kind[i / 2];
    if (kind == RESNMTF_TIMED_XG) { h->timing.xg_ms_total += ms; h->timing.xg_launches++; }
    else if (kind == RESNMTF_TIMED_XTF) { h->timing.xtf_ms_total += ms; h->timing.xtf_launches++; }
    if (kind >= 0 && kind < RESNMTF_TIMED_KINDS) { h->ktime_ms[kind] += ms; h->klaunch[kind]++; }
  }
  h->ev_used = 0;
  return RESNMTF_OK;
}

// sizes a streaming pass.  Measured on MI355X (tools/sweep_pass.py, tools/stamps.py, tools/micro/):
// 8 waves per workgroup.  `slots` = workgroups the device holds at once (CUs x resident workgroups
// per CU, minus the k x k / aux workgroups of the launch).
//   * one-round geometry: if the whole pass fits the slots with splits of at most 2048 rows, use
//     floor(slots / ntiles) equal splits -- every workgroup is resident from t = 0, none waits for a
//     slot and no CU is left with half the work of its neighbour (the quantisation that cost the
//     628-workgroup / 255-slot X.G launch of c2 a third of its time);
//   * otherwise 16-step workgroups (512 rows; longer for k > 32) that the dispatcher streams through
//     the slots.
// Splits are capped at 16, the depth of the consumer's prefetch.
void size_pass(int NT, int ntiles, int rows_pad, int slots, int max_nw, int force_nw, int force_ns, bool fine,
               int* nsplit, int* rps, int* nw) {
  int w = std::min(8, max_nw);
  if (max_nw > 8 && (force_nw == 4 || force_nw == 8 || force_nw == 16)) w = force_nw;
  const int quantum = 4 * w * 8;                       // rows of one unrolled trip of a workgroup
  // streamed geometry: 16-step workgroups (512 rows); for k > 32 only about 8 workgroups per slot, i.e.
  // longer splits -- there the per-workgroup epilogue (tree sum of 64 accumulator registers per lane +
  // slab store) costs as much as several trips (c5 X.G pass: 744 -> 602 us; k <= 32 prefers short splits)
  // k > 16 (pass_body_k32): a workgroup trip is 256 rows, so splits are whole trips where the extent allows
  // k <= 16, f32 image: a split is any whole number of 4 w-row steps (the ragged last trip is masked), so splits come out
  // nearly equal -- c2 X^T.F: 15 x 672 rows instead of 14 x 704 + 192.  Measured neutral (16.4 us either way: with 480
  // workgroups in flight the launch runs at what the memory system delivers, 5.3 TB/s between ramp and drain); kept for
  // the even timeline.  The 2-byte images step in 16 w rows and keep 64
  const int gran = NT >= 2 ? quantum : (fine ? 4 * w : 64);
  int r = 2 * quantum;
  if (NT >= 3) {
    const int ns_stream = std::max(1, std::min(16, ceil_div(8 * (slots + 1), std::max(ntiles, 1))));
    r = std::max(r, round_up(ceil_div(rows_pad, ns_stream), gran));
  }
  if (ceil_div(rows_pad, r) > 16) r = round_up(ceil_div(rows_pad, 16), quantum);
  const int ns_one = std::min(16, slots / std::max(ntiles, 1));
  if (ns_one >= 1) {
    const int r_one = round_up(ceil_div(rows_pad, ns_one), gran);
    if (r_one <= 2048 && r_one >= quantum) r = r_one;
  }
  if (force_ns > 0) r = round_up(ceil_div(rows_pad, force_ns), 64);
  r = std::min(r, round_up(rows_pad, 64));
  *rps = r;
  *nsplit = ceil_div(rows_pad, r);
  *nw = w;
}
// k > 16, wide form (pass_body_wide): a workgroup = TW tiles x 8 / TW row groups, one workgroup per CU.  Picks TW in
// {8, 4} and the number of row splits (<= 16, the depth of the consumer's prefetch) so that the grid fills whole rounds
// of the CUs -- 294 workgroups on 256 CUs cost a c5 X.G pass 468 us against 343 us with 490 (tools/micro/pass_k32_lab.hip)
// -- preferring wide workgroups (the B block is read once per workgroup) and few splits (slab traffic).
void size_aux(int rows_pad, int nw, int max_splits, int* nsplit, int* rps);
// k > 16, wide form (pass_body_wide): a workgroup = TW tiles x 8 / TW row groups, one workgroup per CU.  Picks TW in
// {8, 4}, the number of row splits (<= 16, the depth of the consumer's prefetch) and -- hand-off mode B -- the row splits
// of the aux tiles by a small model of the launch: main workgroups of equal length dealt greedily to the CUs as they
// become free, the aux workgroups (they head the grid) holding one CU each for t_aux and the k x k job one more for
// t_kk behind the last of them.  What the model has to get right (tools/stamps.py, tools/micro/pass_k32_lab.hip on c5):
//   * 294 main workgroups on 256 CUs are two rounds, the second almost empty: 468 us against 343 us with 490;
//   * 32 aux workgroups of 45-100 us in front of 240 main ones: 16 main workgroups start that much later, and the one
//     that gets the k x k job's CU started at 184 us and ended the launch at 442 us where the others ended at 320;
//   * CUs that only ran an aux workgroup idle for the rest of a one-round launch.
// Fewer splits mean less slab traffic (2 KP / rows of the X bytes per split) and fewer per-workgroup prologues.
struct WidePlan { int tw = 8, nsplit = 1, rps = 64, nsaux = 1, rpsaux = 64; double makespan = 1e300; };
// Workgroups are dealt round-robin to the 8 XCDs whatever their load (MI355X_MICROARCH.md, Workgroup dispatch): XCD x
// serves the workgroups i = x (mod 8) of the grid, in order, with ITS CUs -- a workgroup starts on the CU of its XCD that
// becomes free first.  Grid order: the aux workgroups (t_aux each; the k x k job keeps the CU of the last one t_kk longer),
// then the main workgroups, split-major; all splits have d_long except the last (d_last).
double wide_makespan(int ntg, int nsplit, double d_long, double d_last, int n_cu, int aux_wgs, double t_aux, double t_kk) {
  const int cus = std::max(1, n_cu / 8);
  std::vector<std::vector<double>> free_at(8, std::vector<double>((size_t)cus, 0.0));
  auto place = [&](int index, double d) {
    std::vector<double>& f = free_at[(size_t)(index & 7)];
    size_t cu = 0;
    for (size_t c = 1; c < f.size(); ++c)
      if (f[c] < f[cu]) cu = c;
    f[cu] += d;
    return f[cu];
  };
  double end = 0.0;
  for (int i = 0; i < aux_wgs; ++i) end = std::max(end, place(i, i == aux_wgs - 1 ? t_aux + t_kk : t_aux));
  for (int s = 0; s < nsplit; ++s)
    for (int g = 0; g < ntg; ++g) end = std::max(end, place(aux_wgs + s * ntg + g, s == nsplit - 1 ? d_last : d_long));
  // (the estimate of the main tiles is pessimistic for views that partly fit the Infinity Cache: keep the aux + k x k
  // path well inside it)
  return std::max(end, aux_wgs > 0 ? 1.5 * (t_aux + t_kk) : 0.0);
}
WidePlan plan_wide(int ntiles, int rows_pad, int KP, int kinds /* aux products, 0 = hand-off mode A */, int n_cu, int force_ns, int nw) {
  const double t_pass = 4.0 * ntiles * 64.0 * rows_pad / 5.0e6;          // us for the X bytes at 5 TB/s
  // the k x k job of the last-arriving aux workgroup (tools/stamps.py, after its slab loads were batched): Xt.F launch (two aux
  // kinds) 6 us at k = 32, 18 at k = 64; X.G launch (three kinds, the S rule and the error inside) 14 / 49 us; hand-off mode A
  // (job in workgroup 0 for the whole launch): the earlier, slower figure
  const double r3 = (KP / 64.0) * (KP / 64.0) * (KP / 64.0);
  // (round 3, k x k products with conflict-free operand reads: 14.8 / 32 us at k = 64, 6 / 13 us at k = 32 -- profiles/r03_stamps_c5_kk.txt)
  const double t_kk = kinds == 3 ? 9.0 + 23.0 * r3 : kinds == 2 ? 4.5 + 10.3 * r3 : 12.0 + 50.0 * r3;
  WidePlan best;
  double best_aux_time = 1e300;
  int last_na = -1;
  for (int want : {1, 2, 3, 4, 5, 6, 8, 10, 12, 16}) {
    int na = 1, ra = 64;
    size_aux(rows_pad, nw, want, &na, &ra);
    if (kinds > 0 && na == last_na) continue;
    last_na = na;
    const int aux_wgs = kinds > 0 ? kinds * na : 1;                       // mode A: workgroup 0 is the k x k job
    const double t_aux = kinds > 0 ? 2.0 * 256.0 * ra / 25.0e3 + 5.0 : 0.0;   // both operands at one CU's ~25 GB/s share
    if (aux_wgs > n_cu / 2) break;
    for (int tw : {8, 4}) {
      const int trip = 32 * (8 / tw), ntg = ceil_div(ntiles, tw);
      for (int ns = 1; ns <= 16; ++ns) {
        if (force_ns > 0 && ns != force_ns) continue;
        // equal splits, or a SHORT last split: its workgroups are the last of the grid and start on the CUs the aux
        // workgroups (and the k x k job) free -- the launch then ends with every CU busy instead of leaving those idle
        for (double last_share : {1.0, 0.85, 0.7, 0.55, 0.4}) {
          // (a short last split is there to fill the CUs the aux workgroups free: about as many workgroups as those)
          if (last_share < 1.0 && (ns < 2 || force_ns > 0 || ntg > aux_wgs + aux_wgs / 2)) continue;
          const int r = round_up((int)std::ceil(rows_pad / (ns - 1 + last_share)), trip);
          const int ns_real = ceil_div(rows_pad, r);
          if (ns_real != ns && force_ns <= 0) continue;                   // (a shorter list of splits is scored under its own count)
          const int r_last = rows_pad - (ns_real - 1) * r;
          const double per_row = t_pass * n_cu * (1.0 + ns_real * 2.0 * KP / rows_pad) * (tw == 8 ? 1.0 : 1.03) / ((double)ntg * rows_pad);   // CU us per row of a workgroup
          const double ms = wide_makespan(ntg, ns_real, per_row * r + 4.0, per_row * r_last + 4.0, n_cu, aux_wgs, t_aux,
                                          kinds > 0 ? t_kk : t_kk + 10.0);
          // ties (within 1 %) go to the plan whose aux workgroups and k x k job are done first: which aux workgroup arrives
          // last -- and hosts the job -- is not known, and a main workgroup that has to wait for that CU in a launch without
          // slack ends it late (c5 X.G with 3 aux workgroups of 180 us: job done at 245 us, last main workgroup 245 -> 395 us
          // where the others ended at 337)
          const bool tie = ms < best.makespan * 1.01 && ms >= best.makespan * 0.99;
          if (tie && t_aux >= best_aux_time) continue;
          if (!tie && ms >= best.makespan) continue;
          best_aux_time = t_aux;
          best.makespan = std::min(ms, best.makespan); best.tw = tw; best.nsplit = ns_real; best.rps = r; best.nsaux = na; best.rpsaux = ra;
        }
      }
    }
    if (kinds == 0) break;
  }
  return best;
}
// (wide form, k > 16: at most 16 -- the k x k job sums the slabs of every split while the pass saturates the memory
// system, and with one workgroup per CU and one or two rounds of long main workgroups its CU is missing for as long as
// it runs: c5 passes 409 / 486 us with 32 / 49 aux splits against 326 / 313 us for the main tiles alone)
void size_aux(int rows_pad, int nw, int max_splits, int* nsplit, int* rps) {
  const int quantum = 4 * nw * 8;
  int r = quantum;
  if (ceil_div(rows_pad, r) > max_splits) r = round_up(ceil_div(rows_pad, max_splits), quantum);
  r = std::min(r, round_up(rows_pad, 64));
  *rps = r;
  *nsplit = ceil_div(rows_pad, r);
}

int sync_both(resnmtf_handle* h) {
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return RESNMTF_OK;
}

// pinned, device-mapped host mirror of the per-sweep errors ([cap][V]) and of the loop control
hipError_t alloc_host_mirrors(resnmtf_handle* h, int cap) {
  if (h->err_host) (void)hipHostFree(h->err_host);
  h->err_host = nullptr; h->err_host_dev = nullptr;
  hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h->err_host), (size_t)cap * h->V * sizeof(double),
                               hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return e;
  std::memset(h->err_host, 0, (size_t)cap * h->V * sizeof(double));
  if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->err_host_dev), h->err_host, 0)) != hipSuccess) return e;
  if (!h->fuse_err) {
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&h->fuse_err), sizeof(int), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return e;
    *h->fuse_err = 0;
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->fuse_err_dev), h->fuse_err, 0)) != hipSuccess) return e;
  }
  if (!h->ctl_host) {
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&h->ctl_host), sizeof(SweepCtl), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return e;
    std::memset(h->ctl_host, 0, sizeof(SweepCtl));
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->ctl_host_dev), h->ctl_host, 0)) != hipSuccess) return e;
  }
  return hipSuccess;
}

int ensure_err_capacity(resnmtf_handle* h, int sweeps) {
  if (sweeps <= h->err_cap) return RESNMTF_OK;
  if (int rc = sync_both(h)) return rc;
  if (h->err) (void)hipFree(h->err);
  h->err = nullptr;
  const int cap = std::max(sweeps, 1024);
  hipError_t e = dev_alloc_zero(&h->err, (size_t)cap * h->V);
  if (e == hipSuccess) e = hipDeviceSynchronize();      // (NULL-stream memset vs the handle's non-blocking stream)
  if (e == hipSuccess) e = alloc_host_mirrors(h, cap);
  if (e != hipSuccess) { h->err_cap = 0; return h->fail_hip("hipMalloc err", e); }
  h->err_cap = cap;
  h->prepared = false;   // kernel argument blocks hold the pointer
  return RESNMTF_OK;
}

}  // namespace

extern "C" {

int resnmtf_abi_version(void) { return RESNMTF_ABI_VERSION; }

int resnmtf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void resnmtf_default_options(resnmtf_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->device_id = 0;
  o->stream = nullptr;
  o->use_graph = 1;
  o->check_every = 32;     // (sweeps after the stop test fired are empty launches: ~2 us each)
}

const char* resnmtf_last_error(const resnmtf_handle* h) {
  return h ? h->last_error.c_str() : g_create_error.c_str();
}

}  // extern "C"
namespace {
// slabs a sparse view's passes may write (the split count is chosen at upload, resnmtf_set_view_csc): at most 4 for X.G keeps
// the views eligible for the fused F chain (f_chain_kernel keeps up to four raw split slabs per view); Xt.F: 16, the
// consumer's prefetch depth, as for the dense passes
constexpr int kSparseMaxSplit[2] = {4, 16};
// what the allocations of a side are called in create's error messages
struct SideNames { const char *factor, *mult, *slab, *image, *sparse; };
constexpr SideNames kNames[2] = {{"F", "lambda", "Pxg", "Xt", "CSR"}, {"G", "mu", "Pxtf", "X", "CSC"}};
int create_impl(int n_views, const int* n_rows, const int* n_cols, const int* k, const int* owned, const long long* nnz_capacity,
                const resnmtf_options* opts, resnmtf_handle** out) {
  if (!out) { g_create_error = "out is NULL"; return RESNMTF_ERR_INVALID; }
  *out = nullptr;
  if (n_views < 1 || !n_rows || !n_cols || !k) { g_create_error = "bad view description"; return RESNMTF_ERR_INVALID; }
  if (n_views > RESNMTF_MAX_COUPLE + 1) { g_create_error = "too many views (max 17)"; return RESNMTF_ERR_INVALID; }
  for (int v = 0; v < n_views; ++v) {
    if (n_rows[v] < 1 || n_cols[v] < 1) { g_create_error = "view dimensions must be positive"; return RESNMTF_ERR_INVALID; }
    if (k[v] < 1 || k[v] > RESNMTF_MAX_K) { g_create_error = "k must be in [1, 64]"; return RESNMTF_ERR_INVALID; }
    if (k[v] > n_cols[v] || k[v] > n_rows[v]) { g_create_error = "k exceeds a view dimension (R/utils.r:444,449)"; return RESNMTF_ERR_INVALID; }
  }
  resnmtf_options o;
  resnmtf_default_options(&o);
  if (opts) {
    if (opts->struct_size != (int)sizeof(resnmtf_options)) { g_create_error = "options struct_size mismatch"; return RESNMTF_ERR_INVALID; }
    o = *opts;
  }
  if (o.pass_splits_xg < 0 || o.pass_splits_xg > 16 || o.pass_splits_xtf < 0 || o.pass_splits_xtf > 16) {
    g_create_error = "pass_splits_xg / pass_splits_xtf must be in 0 ... 16 (0 = the launch model's choice)";      // (a forced count beyond
    return RESNMTF_ERR_INVALID;                                                                          //  the planner's range found no plan)
  }
  if (o.target_workgroups != 0 && o.target_workgroups < 64) {      // (the launch planner needs room for the aux workgroups of the k > 16 passes)
    g_create_error = "target_workgroups must be 0 (the device's own figure) or at least 64";
    return RESNMTF_ERR_INVALID;
  }
  if (o.bf16_split == 1) { g_create_error = "bf16_split = 1 (the two-piece form) is retired: use 0 (three pieces, f32-grade) or 2 (f32 MFMA)"; return RESNMTF_ERR_INVALID; }
  if (o.slice_chains) {
    const char* why = nullptr;
    if (!o.replicate_f || !o.replicate_gs) why = "slice_chains needs replicate_f and replicate_gs";
    else if (o.slice_count != n_views || n_views < 1 || n_views > 8) why = "slice_chains needs slice_count = number of views <= 8";
    else if (o.slice_index < 0 || o.slice_index >= o.slice_count) why = "slice_index out of range";
    else if (o.x_half != 0 || o.kk_mode == 1) why = "slice_chains uses the f32 images and hand-off mode B";
    else if (!owned) why = "slice_chains needs exactly one owned view (view index = slice_index)";
    else
      for (int v = 0; v < n_views && !why; ++v) {
        if (n_rows[v] != n_rows[0] || n_cols[v] != n_cols[0] || k[v] != k[0]) why = "slice_chains needs equal shapes and k in all views";
        else if ((owned[v] != 0) != (v == o.slice_index)) why = "slice_chains needs exactly one owned view (view index = slice_index)";
      }
    if (why) { g_create_error = why; return RESNMTF_ERR_INVALID; }
  }
  if (o.slice_p2p && !o.slice_chains) {      // peer stores for the exchange blocks of the replicated layouts
    const char* why = nullptr;
    if (!o.replicate_f) why = "slice_p2p needs slice_chains or the replicated chains (replicate_f)";
    else if (o.slice_count != n_views || n_views < 1 || n_views > 8) why = "slice_p2p needs slice_count = number of views <= 8";
    else if (o.slice_index < 0 || o.slice_index >= o.slice_count) why = "slice_index out of range";
    else if (!owned) why = "slice_p2p needs exactly one owned view (view index = slice_index)";
    else
      for (int v = 0; v < n_views && !why; ++v)
        if ((owned[v] != 0) != (v == o.slice_index)) why = "slice_p2p needs exactly one owned view (view index = slice_index)";
    if (why) { g_create_error = why; return RESNMTF_ERR_INVALID; }
  }
  if (nnz_capacity) {
    bool any = false;
    for (int v = 0; v < n_views; ++v) any = any || nnz_capacity[v] >= 0;
    if (any && (o.replicate_f || o.replicate_gs || o.slice_chains || o.slice_p2p)) {
      g_create_error = "sparse views are not supported by the view-sharded layouts (replicate_f / replicate_gs / slice_chains / slice_p2p)";
      return RESNMTF_ERR_INVALID;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    g_create_error = "no HIP device available (this library has no CPU fallback)";
    return RESNMTF_ERR_NO_DEVICE;
  }
  if (o.device_id < 0 || o.device_id >= ndev) { g_create_error = "device_id out of range"; return RESNMTF_ERR_INVALID; }
  hipError_t e = hipSetDevice(o.device_id);
  if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  hipDeviceProp_t prop;
  int n_cu = 256;
  if (hipGetDeviceProperties(&prop, o.device_id) == hipSuccess) {
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      g_create_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
      return RESNMTF_ERR_NO_DEVICE;
    }
    if (prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
  }
  auto* h = new resnmtf_handle();
  h->n_cu = n_cu;
  h->V = n_views;
  h->opt = o;
  if (h->opt.check_every < 1) h->opt.check_every = 8;
  h->views.resize(n_views);
  h->phi.assign((size_t)n_views * n_views, 0.0);
  h->xi = h->phi;
  h->psi = h->phi;
  for (int v = 0; v < n_views; ++v) {
    ViewState& vs = h->views[v];
    vs.n = n_rows[v]; vs.m = n_cols[v]; vs.k = k[v];
    vs.NT = ceil_div(k[v], 16); vs.KP = 16 * vs.NT;
    vs.n_pad = round_up(vs.n, 64); vs.m_pad = round_up(vs.m, 64);
    // tile-major images: tile t of side s's image = its lines 64 t .. 64 t + 63 as [other side's pad][64], contiguous; one
    // extra 256-B row per tile keeps the tile starts off a common power-of-two stride (memory channels)
    const size_t pad_rows = o.no_pitch_pad ? 0 : 1;
    for (int s = 0; s < 2; ++s) {
      Side& sd = vs.side[s];
      sd.len = s == SIDE_F ? vs.n : vs.m; sd.pad = round_up(sd.len, 64);
      sd.ldx = ((size_t)(s == SIDE_F ? vs.m_pad : vs.n_pad) + pad_rows) * 64; sd.x_floats = (size_t)(sd.pad / 64) * sd.ldx;
      sd.map.resize(n_views);
    }
    vs.owned = owned ? owned[v] != 0 : true;
    vs.sparse = nnz_capacity && nnz_capacity[v] >= 0;
    vs.nnz_cap = vs.sparse ? nnz_capacity[v] : 0;
    if (!vs.owned) h->all_owned = false;
    else h->last_owned = v;
  }
  auto bail = [&](hipError_t err, const std::string& what) {
    g_create_error = what + ": " + hipGetErrorString(err);
    resnmtf_destroy(h);
    return err == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  };
  if (o.stream) { h->stream = reinterpret_cast<hipStream_t>(o.stream); h->own_stream = false; }
  else {
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return bail(e, "hipStreamCreate");
    h->own_stream = true;
  }
  if ((e = dev_alloc_zero(&h->ctl, 1)) != hipSuccess) return bail(e, "hipMalloc ctl");
  h->err_cap = 1024;
  if ((e = dev_alloc_zero(&h->err, (size_t)h->err_cap * n_views)) != hipSuccess) return bail(e, "hipMalloc err");
  if ((e = alloc_host_mirrors(h, h->err_cap)) != hipSuccess) return bail(e, "hipHostMalloc error mirror");
  // replicate_f / replicate_gs: one arena per side holds that side's exchange block of every view, in view order
  // (equal-shaped views give equal strides, so that one in-place all-gather moves every rank's block -- sharded.py)
  const bool replicated[2] = {o.replicate_f != 0, o.replicate_gs != 0};
  auto sum_bytes = [](const ViewState& vs, int s) { return ((size_t)vs.side[s].pad * vs.KP * sizeof(float) + 255) / 256 * 256; };
  auto blk_size = [&](const ViewState& vs, int s) {
    return (sum_bytes(vs, s) + (2 * (size_t)vs.k * vs.k + (size_t)vs.k) * sizeof(double) + 255) / 256 * 256;
  };
  if (o.replicate_gs) {
    if (!o.replicate_f) { g_create_error = "replicate_gs needs replicate_f"; resnmtf_destroy(h); return RESNMTF_ERR_INVALID; }
    for (const auto& vs : h->views)
      if (vs.k != h->views[0].k) { g_create_error = "replicate_gs needs the same k in every view"; resnmtf_destroy(h); return RESNMTF_ERR_INVALID; }
  }
  // replicate_gs, equal-shaped F blocks: the S block of a view (k x k inputs of the S rule, written by the same pass launch
  // that produces U) is appended to its F block, so that ONE all-gather after the X.G pass moves both -- two collectives per
  // sweep between dependent steps instead of three
  const size_t kk0 = (size_t)h->views[0].k * h->views[0].k;
  if (o.replicate_gs) h->sblk_stride = (5 * kk0 + 2 * (size_t)h->views[0].k + 1 + 31) / 32 * 32;
  size_t sblk_tail_bytes = 0;
  if (o.replicate_f && o.replicate_gs && !o.slice_chains) {      // (sliced chains: the S blocks travel on their own, beside the U slices)
    bool equal = true;
    for (const auto& vs : h->views) equal = equal && blk_size(vs, SIDE_F) == blk_size(h->views[0], SIDE_F) && vs.k == h->views[0].k;
    if (equal) {
      sblk_tail_bytes = (h->sblk_stride * sizeof(double) + 255) / 256 * 256;
      h->sblk_embedded = true;
    }
  }
  for (int s = 0; s < 2; ++s) {
    if (!replicated[s]) continue;
    for (const auto& vs : h->views) h->arena_bytes[s] += blk_size(vs, s) + (s == SIDE_F ? sblk_tail_bytes : 0);
    if ((e = hipMalloc(&h->arena[s], h->arena_bytes[s])) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].factor + " exchange blocks");
    if ((e = hipMemset(h->arena[s], 0, h->arena_bytes[s])) != hipSuccess) return bail(e, std::string("hipMemset ") + kNames[s].factor + " exchange blocks");
  }
  if (o.replicate_gs) {
    if (!h->sblk_embedded) {
      if ((e = dev_alloc_zero(&h->sblk_arena, h->sblk_stride * n_views)) != hipSuccess) return bail(e, "hipMalloc S exchange blocks");
      h->sblk_base = h->sblk_arena; h->sblk_step = h->sblk_stride;
    }
    if ((e = dev_alloc_zero(&h->view_sweep, (size_t)n_views + 1)) != hipSuccess) return bail(e, "hipMalloc view_sweep");
  }
  if (o.slice_chains) {
    const ViewState& v0 = h->views[0];
    const int V = n_views;
    h->sliced = true;
    for (int s = 0; s < 2; ++s) {
      h->sl_len[s] = round_up(ceil_div(v0.side[s].len, V), 32);
      h->p_chunk[s] = (size_t)h->sl_len[s] * v0.KP * sizeof(float);
      if (s == SIDE_G) h->p_chunk[s] = (h->p_chunk[s] + 2 * (size_t)v0.k * v0.k * sizeof(double) + 255) / 256 * 256;      // (+ the tail Ma_G | Md_G)
      for (char** buf : {&h->p_send[s], &h->p_recv[s]}) {
        if ((e = hipMalloc(reinterpret_cast<void**>(buf), h->p_chunk[s] * V)) != hipSuccess) return bail(e, "hipMalloc slice exchange buffers");
        if ((e = hipMemset(*buf, 0, h->p_chunk[s] * V)) != hipSuccess) return bail(e, "hipMemset slice exchange buffers");
      }
      for (float** buf : {&h->w_send[s], &h->w_recv[s]})
        if ((e = dev_alloc_zero(buf, (size_t)V * h->sl_len[s] * v0.KP)) != hipSuccess) return bail(e, "hipMalloc slice exchange buffers");
    }
    if ((e = dev_alloc_zero(&h->slice_nd, (size_t)V * 2 * (size_t)round_up(std::max(h->sl_len[SIDE_F], h->sl_len[SIDE_G]), 16) * v0.KP)) != hipSuccess)
      return bail(e, "hipMalloc slice product scratch");
  }
  if (o.slice_p2p) {
    int can = 0;
    (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, o.device_id);
    if (!can) { g_create_error = "slice_p2p needs hipStreamWaitValue32 (hipDeviceAttributeCanUseStreamWaitValue)"; resnmtf_destroy(h); return RESNMTF_ERR_NO_DEVICE; }
    // the arrival counters are written by other devices' atomics and polled by this device's command processor: fine-grained
    // (coherent) memory where the runtime offers it
    if (hipExtMallocWithFlags(reinterpret_cast<void**>(&h->p2p_flags), 64 * sizeof(unsigned int), hipDeviceMallocFinegrained) != hipSuccess) {
      (void)hipGetLastError();
      h->p2p_flags = nullptr;
      if ((e = hipMalloc(reinterpret_cast<void**>(&h->p2p_flags), 64 * sizeof(unsigned int))) != hipSuccess) return bail(e, "hipMalloc p2p flags");
    }
    if ((e = hipMemset(h->p2p_flags, 0, 64 * sizeof(unsigned int))) != hipSuccess) return bail(e, "hipMemset p2p flags");
    h->peers.resize((size_t)n_views);
    h->block_p2p = !o.slice_chains;
  }
  const int force_ns[2] = {o.pass_splits_xg, o.pass_splits_xtf};
  size_t blk_off[2] = {0, 0};
  for (int v = 0; v < n_views; ++v) {
    ViewState& vs = h->views[v];
    const size_t kk = (size_t)vs.k * vs.k, kkp = (size_t)vs.KP * vs.KP;
    for (int s = 0; s < 2; ++s)
      if ((e = dev_alloc_zero(&vs.side[s].W, (size_t)vs.side[s].len * vs.k)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].factor);
    if ((e = dev_alloc_zero(&vs.S, kk)) != hipSuccess) return bail(e, "hipMalloc S");
    // ---- geometry (identical on every rank for a given view: n, m, k and the options decide it)
    // k x k mode (kernels.hip.inc, pass_kernel).  A (k <= 16): the update kernels emit fp64 partial
    // Grams (1-4 KB per workgroup), the job is workgroup 0 of the next pass launch and runs beside the
    // whole pass.  B (k > 16, where those partials would be 8-32 KB per workgroup): MFMA aux tiles in
    // the pass launch, tiny slab volume at any k, the job starts once the aux workgroups are done and
    // hides behind the (long) pass.  Measured on c2 ... 40000 x 2000 / 10000 x 8000 (tools/tune_c2.py):
    // A wins at k = 16 for every size tried; B wins at k = 32 / 64 (tools/bench_configs.py).
    const size_t xbytes = (size_t)vs.n * vs.m * sizeof(float);
    vs.kk_mode = (vs.KP == 16) ? 0 : 1;
    if (o.kk_mode == 1) vs.kk_mode = 0;
    if (o.kk_mode == 2 || o.slice_chains) vs.kk_mode = 1;      // (sliced chains: the Gram products come from the received f32 copy)
    if (vs.sparse) vs.kk_mode = 0;                              // (sparse views: mode A at every k, the job in the spmm launch)
    // workgroup slots of a pass launch: target_workgroups overrides CUs x resident workgroups per CU
    const int nw_guess = (vs.NT <= 1 && (o.pass_waves == 4 || o.pass_waves == 8 || o.pass_waves == 16)) ? o.pass_waves : 8;
    const bool wide = vs.NT >= 2 && o.bf16_split != 2;          // k > 16: the wide bf16-piece form
    const int aux_cap = wide ? 16 : 64;
    const int slots_all = o.target_workgroups > 0 ? o.target_workgroups : h->n_cu * pass_blocks_per_cu(vs.NT, nw_guess);
    const bool fine = o.x_half == 0;
    const int RG = update_threads(vs.KP) / vs.KP;
    // update workgroups: mode A ~160 (few partials for the k x k job, two prefetched row groups each
    // at c2 -- tools/tune_c2.py); mode B (k > 16) ONE round of resident workgroups -- one 1024-thread workgroup per CU
    // at k > 32 (127 KB of LDS), two 512-thread ones at k = 32: every workgroup first copies the two k x k coefficient
    // matrices into LDS (64 KB at k = 64, 13 of the 61 us of a c5-sized F update when three rounds of workgroups each
    // did it: tools/ab_update_blocks.sh, F update 61 -> 43 us at c5, 13.5 -> 11.8 at c4; G 19 -> 14.5 at c5)
    const int nblk_round = h->n_cu * (update_threads(vs.KP) >= 1024 ? 1 : 2);
    const int nblk_target = o.update_blocks > 0 ? o.update_blocks : (vs.kk_mode == 0 ? (xbytes <= ((size_t)256 << 20) ? 160 : 512) : nblk_round);
    for (int s = 0; s < 2; ++s) {      // the pass that feeds side s: pad / 64 tiles, reduction over the other side's lines
      Side& sd = vs.side[s];
      const int ntiles = sd.pad / 64, rows_pad = vs.side[other(s)].pad;
      const int kinds = vs.kk_mode == 0 ? 0 : kAuxKinds[s];
      size_aux(rows_pad, nw_guess, aux_cap, &sd.nsaux, &sd.rpsaux);
      const int slots = slots_all - (kinds == 0 ? 1 : kinds * sd.nsaux);
      size_pass(vs.NT, ntiles, rows_pad, slots, max_pass_waves(vs.NT), o.pass_waves, force_ns[s], fine, &sd.nsplit, &sd.rps, &sd.nw);
      if (wide) {
        const WidePlan pw = plan_wide(ntiles, rows_pad, vs.KP, kinds, slots_all, force_ns[s], nw_guess);
        sd.tw = pw.tw; sd.nsplit = pw.nsplit; sd.rps = pw.rps;
        if (kinds != 0) { sd.nsaux = pw.nsaux; sd.rpsaux = pw.rpsaux; }
      }
      // k <= 16: when the workgroups of a pass outnumber the slots (streamed geometry) each wave keeps the next
      // trip's loads in flight while it multiplies (two buffers of 4 steps instead of one of 8): X.G pass of a
      // 40000 x 2000 view 74 -> 67 us.  With everything resident from t = 0 (c2) the plain form is faster.
      sd.pp = vs.NT == 1 && sd.nw == 8 && ntiles * sd.nsplit > slots;
      if (vs.sparse) { sd.nsplit = kSparseMaxSplit[s]; sd.pp = false; }   // (slab capacity; set at upload)
      sd.rpb = round_up(std::max(RG, ceil_div(sd.len, nblk_target)), RG); sd.nblk = ceil_div(sd.len, sd.rpb);
    }
    // mode A: fp64 partials of the update workgroups (G: the cross product T^T G beside the Gram)
    auto part_count = [&](int s) { return (size_t)vs.side[s].nblk * ((s == SIDE_F ? 1 : 2) * kkp + vs.KP); };
    // ---- the updates' inputs.  replicate_f / replicate_gs: one contiguous exchange block per view and side, on every rank
    // (the sharded driver broadcasts it from the owner and runs the update of coupled views everywhere)
    for (int s = 0; s < 2; ++s) {
      if (!replicated[s]) continue;
      Side& sd = vs.side[s];
      sd.xblk_bytes = blk_size(vs, s) + (s == SIDE_F ? sblk_tail_bytes : 0);
      char* base = static_cast<char*>(h->arena[s]) + blk_off[s];
      blk_off[s] += sd.xblk_bytes;
      sd.xblk = base;
      sd.xsum = reinterpret_cast<float*>(base);
      sd.Ma = reinterpret_cast<double*>(base + sum_bytes(vs, s));
      sd.Md = sd.Ma + kk;
      sd.lm = sd.Md + kk;
      if (s == SIDE_F && h->sblk_embedded) {
        vs.sblk = reinterpret_cast<double*>(base + blk_size(vs, s));
        if (v == 0) { h->sblk_base = vs.sblk; h->sblk_step = sd.xblk_bytes / sizeof(double); }
      }
      if (s == SIDE_G && !h->sblk_embedded) vs.sblk = h->sblk_arena + (size_t)v * h->sblk_stride;
      if (!vs.owned) {                // (a replica writes the same copies as the owner: nobody reads them here)
        sd.replica = true;
        if ((e = dev_alloc_zero(&sd.W32, (size_t)sd.pad * 64)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].factor + "32");
        if (s == SIDE_G && (e = dev_alloc_zero(&vs.T32, (size_t)sd.pad * 64)) != hipSuccess) return bail(e, "hipMalloc T32");
        if (vs.kk_mode == 0 && (e = dev_alloc_zero(&sd.part, part_count(s))) != hipSuccess) return bail(e, std::string("hipMalloc part") + kNames[s].factor);
      }
    }
    if (!vs.owned) continue;
    vs.half = !vs.sparse && (o.x_half >= 1 && o.x_half <= 3) && vs.NT == 1 && vs.kk_mode == 0 && vs.side[SIDE_F].nw == 8 && vs.side[SIDE_G].nw == 8;
    vs.u16 = vs.half && o.x_half >= 2;
    vs.half_capable = vs.half;
    for (int s = 0; s < 2; ++s) {
      Side& sd = vs.side[s];
      if ((e = dev_alloc_zero(&sd.P, (size_t)sd.nsplit * sd.pad * vs.KP)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].slab);
      if (!replicated[s]) {
        if ((e = dev_alloc_zero(&sd.lm, (size_t)vs.k)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].mult);
        for (double** pp : {&sd.Ma, &sd.Md})
          if ((e = dev_alloc_zero(pp, kk)) != hipSuccess) return bail(e, "hipMalloc kxk");
      }
      if (vs.sparse) {                // CSC + CSR at the declared capacity, no dense image (x_half never applies)
        const size_t cap = (size_t)std::max<long long>(vs.nnz_cap, 1);
        if ((e = dev_alloc_zero(&sd.sp_ptr, (size_t)sd.len + 1)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].sparse + " pointers");
        if ((e = dev_alloc_zero(&sd.sp_idx, cap)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].sparse + " indices");
        if ((e = dev_alloc_zero(&sd.sp_val, cap)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].sparse + " values");
      } else if ((e = dev_alloc_zero(&sd.X, sd.x_floats)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].image + "32");
      if (vs.half) {      // one spare row group per tile keeps the tile starts off a common power-of-two stride
        sd.ld16 = ((size_t)vs.side[other(s)].pad + 4) * 64; sd.x16_halves = (size_t)(sd.pad / 64) * sd.ld16;
        if ((e = dev_alloc_zero(&sd.X16, sd.x16_halves)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].image + "16");
      }
      if ((e = dev_alloc_zero(&sd.W32, (size_t)sd.pad * 64)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].factor + "32");
      if (vs.NT >= 2 && (e = dev_alloc_zero(&sd.Wk, (size_t)sd.pad * vs.KP * 3)) != hipSuccess) return bail(e, std::string("hipMalloc ") + kNames[s].factor + "k");
      if ((e = dev_alloc_zero(&sd.cnt, 4)) != hipSuccess) return bail(e, "hipMalloc cnt");
      if ((e = dev_alloc_zero(&sd.Paux, (size_t)kAuxKinds[s] * sd.nsaux * 64 * vs.KP)) != hipSuccess) return bail(e, "hipMalloc Paux");
      if (vs.kk_mode == 0 && (e = dev_alloc_zero(&sd.part, part_count(s))) != hipSuccess) return bail(e, std::string("hipMalloc part") + kNames[s].factor);
    }
    if ((e = dev_alloc_zero(&vs.xnorm2, 1)) != hipSuccess) return bail(e, "hipMalloc xnorm2");
    if ((e = dev_alloc_zero(&vs.T32, (size_t)vs.m_pad * 64)) != hipSuccess) return bail(e, "hipMalloc T32");
    if ((e = dev_alloc_zero(&vs.fuse_cnt, 4)) != hipSuccess) return bail(e, "hipMalloc cnt");
    for (double** pp : {&vs.FtF, &vs.FtFS})
      if ((e = dev_alloc_zero(pp, kk)) != hipSuccess) return bail(e, "hipMalloc kxk");
    if ((e = dev_alloc_zero(&vs.cF, (size_t)vs.k)) != hipSuccess) return bail(e, "hipMalloc cF");
  }
  if ((e = set_all_attrs()) != hipSuccess) return bail(e, "hipFuncSetAttribute");
  // the zero fills above ran on the NULL stream, which the handle's (non-blocking) stream does not wait
  // for: finish them before anything is enqueued there (a late memset would wipe uploaded data)
  if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(e, "hipDeviceSynchronize");
  if (o.time_kernels) {
    h->ev.resize(8192);
    h->ev_kind.resize(4096);
    for (auto& evt : h->ev)
      if ((e = hipEventCreate(&evt)) != hipSuccess) return bail(e, "hipEventCreate");
  }
  *out = h;
  return RESNMTF_OK;
}
}  // namespace
extern "C" {

int resnmtf_create(int n_views, const int* n_rows, const int* n_cols, const int* k, const int* owned,
                   const resnmtf_options* opts, resnmtf_handle** out) {
  return create_impl(n_views, n_rows, n_cols, k, owned, nullptr, opts, out);
}
int resnmtf_create_sparse(int n_views, const int* n_rows, const int* n_cols, const int* k, const int* owned,
                          const long long* nnz_capacity, const resnmtf_options* opts, resnmtf_handle** out) {
  if (!nnz_capacity) {
    if (out) *out = nullptr;
    g_create_error = "nnz_capacity is NULL (use resnmtf_create for dense views only)";
    return RESNMTF_ERR_INVALID;
  }
  return create_impl(n_views, n_rows, n_cols, k, owned, nnz_capacity, opts, out);
}

int resnmtf_destroy(resnmtf_handle* h) {
  if (!h) return RESNMTF_OK;
  (void)hipSetDevice(h->opt.device_id);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  destroy_graphs(h);
  for (auto& v : h->views) free_view(v);
  if (h->arena[SIDE_F]) (void)hipFree(h->arena[SIDE_F]);
  if (h->arena[SIDE_G]) (void)hipFree(h->arena[SIDE_G]);
  if (h->sblk_arena) (void)hipFree(h->sblk_arena);
  for (auto& pc : h->peers)
    for (void* q : pc.opened)
      if (q) (void)hipIpcCloseMemHandle(q);
  for (void* p : {(void*)h->slice_nd, (void*)h->p2p_flags, (void*)h->view_sweep, (void*)h->p_send[SIDE_F], (void*)h->p_recv[SIDE_F], (void*)h->p_send[SIDE_G], (void*)h->p_recv[SIDE_G], (void*)h->w_send[SIDE_F],
                  (void*)h->w_recv[SIDE_F], (void*)h->w_send[SIDE_G], (void*)h->w_recv[SIDE_G]})
    if (p) (void)hipFree(p);
  if (h->ctl) (void)hipFree(h->ctl);
  if (h->err) (void)hipFree(h->err);
  if (h->err_host) (void)hipHostFree(h->err_host);
  if (h->ctl_host) (void)hipHostFree(h->ctl_host);
  if (h->fuse_err) (void)hipHostFree(h->fuse_err);
  for (auto& evt : h->ev)
    if (evt) (void)hipEventDestroy(evt);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return RESNMTF_OK;
}

namespace {
// fp16 images of an uploaded view: per-view power-of-two scale that puts the largest entry near 2^14
// relative quantisation error of X below which the guarded mode (x_half = 3) lets the passes use the 16-bit image:
// F / G move by 0.2 ... 2 x that error (tools/quant_study.py), the bar is 1e-4
constexpr double kHalfGuard = 3.0e-5;
int build_half_images(resnmtf_handle* h, ViewState& vs) {
  Scratch sc;
  double* scratch = sc.take<double>(3);          // [0] = max entry bits (as unsigned), [1] = sum (x~ - x)^2, [2] = copy of ||X||^2
  if (!scratch) return h->fail_hip("2-byte images (hipMalloc)", sc.error());
  hipError_t e = hipMemsetAsync(scratch, 0, 3 * sizeof(double), h->stream);
  unsigned int bits = 0;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(max_entry_kernel, dim3(1024), dim3(256), 0, h->stream, vs.side[SIDE_G].X, vs.side[SIDE_G].x_floats,
                       reinterpret_cast<unsigned int*>(scratch));
    e = hipMemcpyAsync(&bits, scratch, sizeof(bits), hipMemcpyDeviceToHost, h->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return h->fail_hip("2-byte images (max)", e);
  float mx;
  std::memcpy(&mx, &bits, sizeof(mx));
  int ex = 0;
  vs.xscale = 1.f;
  if (mx > 0.f && std::isfinite(mx)) {
    (void)std::frexp(mx, &ex);
    // fp16: power of two, max * scale in [2^13, 2^14) (exact scaling); integers: the full range, max -> 65535 (the
    // widening is exact whatever the step, the step is taken out once per output in f32)
    vs.xscale = vs.u16 ? 65535.f / mx : std::ldexp(1.f, 14 - ex);
  }
  // the squared quantisation error: one partial per block of the first pack, then a fixed-order sum (no float atomics: the
  // figure resnmtf_view_image_info reports is the same on every run and for every route that left the same image)
  const unsigned pack_blocks = (unsigned)(((size_t)(vs.n_pad / 4) * 64 * (vs.m_pad / 64) + 255) / 256);
  double* sq_part = sc.take<double>(pack_blocks);
  if (!sq_part) return h->fail_hip("2-byte images (hipMalloc)", sc.error());
  hipLaunchKernelGGL(pack_half_kernel, dim3(pack_blocks), dim3(256), 0,
                     h->stream, vs.side[SIDE_G].X, vs.side[SIDE_G].ldx, vs.n_pad, vs.m_pad / 64, vs.xscale, vs.side[SIDE_G].X16, vs.side[SIDE_G].ld16, vs.u16 ? 1 : 0, sq_part);
  hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, h->stream, sq_part, (int)pack_blocks, scratch + 1);
  hipLaunchKernelGGL(pack_half_kernel, dim3((unsigned)(((size_t)(vs.m_pad / 4) * 64 * (vs.n_pad / 64) + 255) / 256)), dim3(256), 0,
                     h->stream, vs.side[SIDE_F].X, vs.side[SIDE_F].ldx, vs.m_pad, vs.n_pad / 64, vs.xscale, vs.side[SIDE_F].X16, vs.side[SIDE_F].ld16, vs.u16 ? 1 : 0,
                     (double*)nullptr);
  double host[2] = {0.0, 0.0};
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&host[0], scratch + 1, sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&host[1], vs.xnorm2, sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return h->fail_hip("2-byte images (pack)", e);
  vs.x_relerr = host[1] > 0.0 ? std::sqrt(host[0] / host[1]) : 0.0;
  const bool use = h->opt.x_half == 3 ? vs.x_relerr <= kHalfGuard : true;
  if (use != vs.half) {               // the factor operand copies follow the image's layout: rewrite them
    vs.half = use;
    if (vs.has_factors) {
      HIP_TRY(h, hipMemsetAsync(vs.side[SIDE_F].W32, 0, (size_t)vs.n_pad * 64 * sizeof(float), h->stream));
      HIP_TRY(h, hipMemsetAsync(vs.side[SIDE_G].W32, 0, (size_t)vs.m_pad * 64 * sizeof(float), h->stream));
      hipLaunchKernelGGL(factor_to_f32_kernel, dim3(ceil_div(vs.n * vs.k, 256)), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n,
                         vs.k, vs.side[SIDE_F].W32, vs.kk_mode == 0 ? vs.KP : 64, vs.NT, vs.half ? 1 : 0, vs.side[SIDE_F].Wk);
      hipLaunchKernelGGL(factor_to_f32_kernel, dim3(ceil_div(vs.m * vs.k, 256)), dim3(256), 0, h->stream, vs.side[SIDE_G].W, vs.m,
                         vs.k, vs.side[SIDE_G].W32, vs.kk_mode == 0 ? vs.KP : 64, vs.NT, vs.half ? 1 : 0, vs.side[SIDE_G].Wk);
      HIP_TRY(h, hipGetLastError());
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
  }
  h->prepared = false;
  h->resume_ok = false;
  return RESNMTF_OK;
}
// ---- the dense upload.  A dense view gets its data from a host matrix, from a shuffle or a sub-sample of another view's
// image (resnmtf_shuffle_view, resnmtf_subsample_view), or from a matrix in the caller's device memory
// (resnmtf_set_view_device): all of them are upload_dense.  It refuses, zeroes the two f32 images,
// lets `enqueue` put the kernels of the route on the handle's stream -- they fill the images and one partial of ||X||^2 per
// 32 x 32 block -- and then sums the partials, reads the flag back and sets the view's state.
// raw = false: x is already non-negative and column-normalised.  raw = true: make_non_neg_inner +
// matrix_normalisation (R/utils.r:20-27, 86-88) run on the device, fused into the conversion.
// Transient device memory: the ceil(n/32) ceil(m/32) block partials and, raw, the 2 m + 1 column statistics, + the route's.
struct DenseUpload {                  // what upload_dense hands to `enqueue`
  Scratch& scratch;                   // the route's own transient buffers come from here too
  dim3 grid;                          // of the convert kernel
  double* partial;
  double *shift, *colsum;             // raw: the column statistics and the was_negative flag (else NULL)
  int* neg;
  int* line_counts;                   // host [2]: device-drawn data reports its all-zero rows / columns here (and in empty_mask)
};
// true when p is device memory of the handle's device; a host pointer makes hipPointerGetAttributes fail (or report host
// memory, by version): both are "no", and the sticky error is cleared
bool on_handle_device(resnmtf_handle* h, const void* p) {
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return attr.type == hipMemoryTypeDevice && attr.device == h->opt.device_id;
}
// the handle's stream waits for everything enqueued on the caller's stream so far
hipError_t wait_for_caller(resnmtf_handle* h, void* stream) {
  hipEvent_t ev = nullptr;
  hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  e = hipEventRecord(ev, static_cast<hipStream_t>(stream));
  if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, ev, 0);
  (void)hipEventDestroy(ev);          // (released once the recorded work completes)
  return e;
}
// device_x: the caller's matrix when the route reads device memory (refused unless it is on the handle's device), else NULL
int upload_dense(resnmtf_handle* h, int v, bool raw, int* was_negative, const void* device_x, const char* what,
                 const std::function<hipError_t(const DenseUpload&)>& enqueue) {
  if (int rc = check_view(h, v)) return rc;
  ViewState& vs = h->views[v];
  if (!vs.owned) return h->fail(RESNMTF_ERR_STATE, "set_view on a view this handle does not own");
  if (vs.sparse) return h->fail(RESNMTF_ERR_INVALID, "the view is sparse: upload it with resnmtf_set_view_csc");
  if (device_x && !on_handle_device(h, device_x))
    return h->fail(RESNMTF_ERR_INVALID, "x is not device memory of the handle's device (host data: resnmtf_set_view / resnmtf_set_view_raw)");
  h->resume_ok = false;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  const dim3 grid(ceil_div(vs.n, 32), ceil_div(vs.m, 32));
  const int nparts = grid.x * grid.y;
  int neg_host = 0, line_counts[2] = {0, 0};
  vs.empty_rows = vs.empty_cols = 0; vs.empty_mask.clear();
  {      // (the transients, the staging image among them, are gone before build_half_images takes its own)
    Scratch sc;
    double* partial = sc.take<double>((size_t)nparts);
    double* colstat = raw ? sc.take<double>((size_t)2 * vs.m + 1) : nullptr;      // [2][m]: shift, colsum; then one int flag
    if (sc.error() != hipSuccess) return h->fail_hip("hipMalloc upload buffers", sc.error());
    int* neg = raw ? reinterpret_cast<int*>(colstat + 2 * (size_t)vs.m) : nullptr;
    hipError_t e = hipMemsetAsync(vs.side[SIDE_G].X, 0, vs.side[SIDE_G].x_floats * sizeof(float), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(vs.side[SIDE_F].X, 0, vs.side[SIDE_F].x_floats * sizeof(float), h->stream);
    if (e == hipSuccess && raw) e = hipMemsetAsync(neg, 0, sizeof(double), h->stream);
    if (e == hipSuccess) e = enqueue(DenseUpload{sc, grid, partial, colstat, raw ? colstat + vs.m : nullptr, neg, line_counts});
    if (e == hipSuccess) {
      hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, h->stream, partial, nparts, vs.xnorm2);
      e = hipGetLastError();
    }
    if (e == hipSuccess && raw) e = hipMemcpyAsync(&neg_host, neg, sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return h->fail_hip(what, e);
  }
  vs.empty_rows = line_counts[0]; vs.empty_cols = line_counts[1];
  if (was_negative) *was_negative = neg_host;
  vs.has_x = true;
  if (vs.half_capable) return build_half_images(h, vs);
  return RESNMTF_OK;
}

// The staged routes: an fp64 image of the view in transient memory (n m doubles), copied from the host matrix x or
// (x == NULL) drawn from another view's device copy -- a pseudo-random permutation of its entries (resnmtf_shuffle_view)
// or a sub-sample (rows != NULL) -- and then which rows / columns of the draw came out all zero.
struct ShuffleSrc { const float* X32; size_t ldx; unsigned long long seed; const int* rows; const int* cols; };   // rows != NULL: sub-sample
int upload_view(resnmtf_handle* h, int v, const double* x, bool raw, int* was_negative, const ShuffleSrc* shuffle_src = nullptr) {
  if (int rc = check_view(h, v)) return rc;
  if (!x && !shuffle_src) return h->fail(RESNMTF_ERR_INVALID, "x is NULL");
  ViewState& vs = h->views[v];
  return upload_dense(h, v, raw, was_negative, nullptr, "set_view", [&](const DenseUpload& u) {
    const size_t count = (size_t)vs.n * vs.m;
    double* staging = u.scratch.take<double>(count);
    unsigned char* line_mask = x ? nullptr : u.scratch.take<unsigned char>((size_t)vs.n + vs.m + 2 * sizeof(int) + 8);
    if (u.scratch.error() != hipSuccess) return u.scratch.error();
    hipError_t e = hipSuccess;
    if (x) e = hipMemcpyAsync(staging, x, count * sizeof(double), hipMemcpyHostToDevice, h->stream);
    else {
      if (shuffle_src->rows)
        hipLaunchKernelGGL(subsample_gather_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, shuffle_src->X32,
                           shuffle_src->ldx, shuffle_src->rows, vs.n, shuffle_src->cols, vs.m, staging);
      else
        hipLaunchKernelGGL(shuffle_gather_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, shuffle_src->X32,
                           shuffle_src->ldx, vs.n, vs.m, shuffle_src->seed, staging);
      e = hipGetLastError();
      int* counts = reinterpret_cast<int*>(line_mask + (((size_t)vs.n + vs.m + 7) / 8) * 8);
      if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 2 * sizeof(int), h->stream);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(empty_lines_kernel, dim3(ceil_div(vs.n + vs.m, 256)), dim3(256), 0, h->stream, staging, vs.n, vs.m, line_mask, counts);
      vs.empty_mask.resize((size_t)vs.n + vs.m);
      e = hipMemcpyAsync(vs.empty_mask.data(), line_mask, (size_t)vs.n + vs.m, hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(u.line_counts, counts, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream);
    }
    if (e != hipSuccess) return e;
    if (raw) hipLaunchKernelGGL(column_stats_kernel, dim3(vs.m), dim3(256), 0, h->stream, staging, vs.n, vs.m, u.shift, u.colsum, u.neg);
    hipLaunchKernelGGL(convert_x_kernel, u.grid, dim3(256), 0, h->stream, staging, vs.n, vs.m, vs.side[SIDE_G].X, vs.side[SIDE_G].ldx,
                       vs.side[SIDE_F].X, vs.side[SIDE_F].ldx, u.partial, u.shift, u.colsum);
    return hipGetLastError();
  });
}

// The device route (resnmtf_set_view_device): no staging image, the kernels of resnmtf_device_view.hip.inc read the
// caller's matrix in place once the handle's stream has waited for the caller's.
int upload_view_device(resnmtf_handle* h, int v, const void* x, int dtype, long long rs, long long cs, bool raw, int* was_negative,
                       void* stream) {
  if (int rc = check_view(h, v)) return rc;
  if (!x) return h->fail(RESNMTF_ERR_INVALID, "x is NULL");
  if (dtype != RESNMTF_DTYPE_F64 && dtype != RESNMTF_DTYPE_F32 && dtype != RESNMTF_DTYPE_F16 && dtype != RESNMTF_DTYPE_BF16)
    return h->fail(RESNMTF_ERR_INVALID, "unknown dtype: one of RESNMTF_DTYPE_F64 / _F32 / _F16 / _BF16");
  if (rs < 0 || cs < 0) return h->fail(RESNMTF_ERR_INVALID, "negative strides are not supported");
  ViewState& vs = h->views[v];
  return upload_dense(h, v, raw, was_negative, x, "set_view_device", [&](const DenseUpload& u) {
    const hipError_t e = wait_for_caller(h, stream);
    if (e != hipSuccess) return e;
    const bool rows = cs == 1 && rs != 1;             // a row-major source: read along c
    pick_int<RESNMTF_DTYPE_F64, RESNMTF_DTYPE_F32, RESNMTF_DTYPE_F16, RESNMTF_DTYPE_BF16>(dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      if (raw) {
        if (rows) hipLaunchKernelGGL(device_column_stats_rows_kernel<DT>, dim3(ceil_div(vs.m, 32)), dim3(256), 0, h->stream, x, rs, vs.n, vs.m, u.shift, u.colsum, u.neg);
        else hipLaunchKernelGGL(device_column_stats_kernel<DT>, dim3(vs.m), dim3(256), 0, h->stream, x, rs, cs, vs.n, vs.m, u.shift, u.colsum, u.neg);
      }
      if (rows) hipLaunchKernelGGL((device_convert_x_kernel<DT, true>), u.grid, dim3(256), 0, h->stream, x, rs, cs, vs.n, vs.m, vs.side[SIDE_G].X,
                                   vs.side[SIDE_G].ldx, vs.side[SIDE_F].X, vs.side[SIDE_F].ldx, u.partial, u.shift, u.colsum);
      else hipLaunchKernelGGL((device_convert_x_kernel<DT, false>), u.grid, dim3(256), 0, h->stream, x, rs, cs, vs.n, vs.m, vs.side[SIDE_G].X,
                              vs.side[SIDE_G].ldx, vs.side[SIDE_F].X, vs.side[SIDE_F].ldx, u.partial, u.shift, u.colsum);
    });
    return hipGetLastError();
  });
}
}  // namespace

int resnmtf_set_view(resnmtf_handle* h, int v, const double* x) { return upload_view(h, v, x, false, nullptr); }
int resnmtf_set_view_raw(resnmtf_handle* h, int v, const double* x_raw, int* was_negative) {
  return upload_view(h, v, x_raw, true, was_negative);
}
int resnmtf_set_view_device(resnmtf_handle* h, int v, const void* x, int dtype, long long row_stride, long long col_stride, int raw,
                            int* was_negative, void* stream) {
  return upload_view_device(h, v, x, dtype, row_stride, col_stride, raw != 0, was_negative, stream);
}

// ---- sparse views
namespace {
// Work blocks of a sparse pass over `lines` output lines with entry pointers ptr.  Every line's entry range is cut into
// nsplit equal pieces (one slab each) and the lines into contiguous blocks of about equal cost (entries + a per-line
// overhead); one wave per (block, piece).  Two forms, chosen per block and fixed here (the bits depend on them):
//   narrow: each group of the wave sums whole lines of the block, side by side (short lines);
//   wide:   every group of the wave takes a fixed stride of ONE line, then an xor butterfly sums the groups.
// Every block is wide when the lines are 2 x groups entries or more on average and too few to give every group of every
// resident wave its own (c2 at 5 %: Xt.F 58 us narrow, 12 us wide; with lines enough narrow is faster: 200000 x 20000 at
// 0.5 %, X.G 276 against 337 us at k = 16, 866 against 1320 us at k = 64).  Otherwise a line much longer than a block's
// share -- a dense row or column among sparse ones -- sits in a block of its own, which runs wide, and nsplit grows until
// one piece of it costs about what a narrow block does: its entries are spread over nsplit waves x all their groups
// instead of one sequential chain.  blk = [nblk + 1 first lines][nblk form flags, 1 = wide].
void plan_sparse(const std::vector<long long>& ptr, int lines, int groups, int n_cu, int max_split, int* nsplit, int* nblk,
                 std::vector<int>& blk) {
  constexpr long long kLine = 4;                       // per-line cost in entries (pointer loads, slab store)
  const long long total = ptr[(size_t)lines] + kLine * lines;
  const long long waves = (long long)n_cu * 16;        // two 8-wave workgroups per CU
  const bool all_wide = ptr[(size_t)lines] >= 2LL * groups * lines && (long long)lines < waves * groups;
  long long maxlen = 0;
  for (int r = 0; r < lines; ++r) maxlen = std::max(maxlen, ptr[(size_t)r + 1] - ptr[(size_t)r]);
  const int g_eff = all_wide ? 1 : groups;             // (all wide: a wave's time per line is its length / groups either way)
  // entries per wave if the launch were spread evenly; a wide piece of L entries costs a wave about what a narrow block
  // of L entries does (both spread over all groups)
  const long long unit = std::max<long long>(16 * g_eff, (total + waves - 1) / waves);
  long long ns = all_wide ? (maxlen + 4 * unit - 1) / (4 * unit) : (maxlen + unit - 1) / unit;
  ns = std::min<long long>(max_split, std::max<long long>(1, ns));
  *nsplit = (int)ns;
  const long long target = std::max<long long>(16 * g_eff, (total * ns + waves - 1) / waves);
  std::vector<int> first(1, 0);
  long long acc = 0;
  for (int r = 0; r < lines; ++r) {
    const long long c = ptr[(size_t)r + 1] - ptr[(size_t)r] + kLine;
    if (acc > 0 && acc + c > target) { first.push_back(r); acc = 0; }
    acc += c;
  }
  first.push_back(lines);
  const int nb = (int)first.size() - 1;
  blk = first;
  for (int b = 0; b < nb; ++b) {
    const bool one_long = first[(size_t)b + 1] - first[(size_t)b] == 1 &&
                          ptr[(size_t)first[(size_t)b] + 1] - ptr[(size_t)first[(size_t)b]] >= 2LL * groups;
    blk.push_back(all_wide || one_long ? 1 : 0);
  }
  *nblk = nb;
}
int spmm_groups_host(int KP) { return KP <= 16 ? 16 : (KP <= 32 ? 8 : 4); }   // = spmm_groups (kernel side)

// The tail every sparse upload shares (resnmtf_set_view_csc, finish_sparse_build, resnmtf_copy_view_sparse) is
// plan_and_commit below.  Its pieces: the work split of the two passes planned from the host copies of the line pointers,
// the block lists (re)allocated and their upload enqueued on the handle's stream (synchronised while `pl` is alive), then
// -- commit_sparse_upload -- the view's state.
struct SparsePlan {
  std::vector<int> bxg, bxtf;
  int ns_xg = 1, ns_xtf = 1, nb_xg = 0, nb_xtf = 0;
};
hipError_t upload_sparse_plan(resnmtf_handle* h, ViewState& vs, const std::vector<long long>& rp, const std::vector<long long>& cp,
                              SparsePlan& pl) {
  const int groups = spmm_groups_host(vs.KP);
  plan_sparse(rp, vs.n, groups, h->n_cu, kSparseMaxSplit[SIDE_F], &pl.ns_xg, &pl.nb_xg, pl.bxg);
  plan_sparse(cp, vs.m, groups, h->n_cu, kSparseMaxSplit[SIDE_G], &pl.ns_xtf, &pl.nb_xtf, pl.bxtf);
  hipError_t e = hipSuccess;
  if (pl.nb_xg != vs.side[SIDE_F].sp_nblk || !vs.side[SIDE_F].sp_blk) {
    if (vs.side[SIDE_F].sp_blk) (void)hipFree(vs.side[SIDE_F].sp_blk);
    vs.side[SIDE_F].sp_blk = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&vs.side[SIDE_F].sp_blk), pl.bxg.size() * sizeof(int));
  }
  if (e == hipSuccess && (pl.nb_xtf != vs.side[SIDE_G].sp_nblk || !vs.side[SIDE_G].sp_blk)) {
    if (vs.side[SIDE_G].sp_blk) (void)hipFree(vs.side[SIDE_G].sp_blk);
    vs.side[SIDE_G].sp_blk = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&vs.side[SIDE_G].sp_blk), pl.bxtf.size() * sizeof(int));
  }
  if (e == hipSuccess) e = hipMemcpyAsync(vs.side[SIDE_F].sp_blk, pl.bxg.data(), pl.bxg.size() * sizeof(int), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(vs.side[SIDE_G].sp_blk, pl.bxtf.data(), pl.bxtf.size() * sizeof(int), hipMemcpyHostToDevice, h->stream);
  return e;
}
void commit_sparse_upload(resnmtf_handle* h, ViewState& vs, const SparsePlan& pl, long long nnz) {
  vs.nnz = nnz;
  vs.side[SIDE_F].sp_nblk = pl.nb_xg; vs.side[SIDE_G].sp_nblk = pl.nb_xtf;
  vs.side[SIDE_F].nsplit = pl.ns_xg; vs.side[SIDE_G].nsplit = pl.ns_xtf;
  vs.has_x = true;
  h->prepared = false;          // the slab count of the updates follows the upload
}
// `e`: the status of what the caller enqueued to fill the view's arrays.  The first synchronisation completes that work
// (and puts rp / cp on the host where the caller read them back), the second one the upload of the block lists.
hipError_t plan_and_commit(resnmtf_handle* h, ViewState& vs, const std::vector<long long>& rp, const std::vector<long long>& cp, long long nnz,
                           hipError_t e) {
  SparsePlan pl;
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = upload_sparse_plan(h, vs, rp, cp, pl);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) commit_sparse_upload(h, vs, pl, nnz);
  return e;
}
}  // namespace

int resnmtf_set_view_csc(resnmtf_handle* h, int v, const long long* col_ptr, const int* row_idx, const double* values,
                         int pre_processed) {
  if (int rc = check_view(h, v)) return rc;
  ViewState& vs = h->views[v];
  if (!vs.sparse) return h->fail(RESNMTF_ERR_INVALID, "the view is dense: upload it with resnmtf_set_view / resnmtf_set_view_raw");
  if (!vs.owned) return h->fail(RESNMTF_ERR_STATE, "set_view_csc on a view this handle does not own");
  if (!col_ptr || !row_idx || !values) return h->fail(RESNMTF_ERR_INVALID, "col_ptr / row_idx / values is NULL");
  const int n = vs.n, m = vs.m;
  // ---- host checks, before any device work
  if (col_ptr[0] != 0) return h->fail(RESNMTF_ERR_INVALID, "col_ptr[0] must be 0 (0-based CSC)");
  for (int j = 0; j < m; ++j)
    if (col_ptr[j + 1] < col_ptr[j]) return h->fail(RESNMTF_ERR_INVALID, "col_ptr is not monotone (column " + std::to_string(j) + ")");
  const long long nnz = col_ptr[m];
  if (nnz > vs.nnz_cap)
    return h->fail(RESNMTF_ERR_INVALID, "col_ptr[m] = " + std::to_string(nnz) + " exceeds the view's nnz capacity " + std::to_string(vs.nnz_cap));
  for (int j = 0; j < m; ++j) {
    double colsum = 0.0;
    for (long long e = col_ptr[j]; e < col_ptr[j + 1]; ++e) {
      const int i = row_idx[e];
      if (i < 0 || i >= n) return h->fail(RESNMTF_ERR_INVALID, "row index out of range in column " + std::to_string(j));
      if (e > col_ptr[j] && i <= row_idx[e - 1])
        return h->fail(RESNMTF_ERR_INVALID, "row indices must be strictly increasing within a column (column " + std::to_string(j) + ")");
      const double x = values[e];
      if (!std::isfinite(x)) return h->fail(RESNMTF_ERR_INVALID, "non-finite entry in column " + std::to_string(j));
      if (x < 0.0)
        return h->fail(RESNMTF_ERR_INVALID, "negative entry in column " + std::to_string(j) +
                       ": make_non_neg (R/utils.r:20-27) shifts a whole column by its minimum, which would turn every implicit zero of a "
                       "sparse view positive -- shift the data on the host and upload it dense");
      colsum += x;
    }
    if (!pre_processed && !(colsum > 0.0))
      return h->fail(RESNMTF_ERR_INVALID, "column " + std::to_string(j) +
                     " is all zero: matrix_normalisation (R/utils.r:86-88) would divide it by zero (a NaN column in the reference)");
  }
  h->resume_ok = false;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  // ---- CSR structure on the host: entries of a row in ascending column order (columns are walked in order)
  std::vector<long long> cp(col_ptr, col_ptr + (size_t)m + 1), rp((size_t)n + 1, 0), perm((size_t)nnz);
  std::vector<int> ci((size_t)nnz);
  for (long long e = 0; e < nnz; ++e) ++rp[(size_t)row_idx[e] + 1];
  for (int i = 0; i < n; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
  {
    std::vector<long long> next(rp.begin(), rp.end() - 1);
    for (int j = 0; j < m; ++j)
      for (long long e = cp[(size_t)j]; e < cp[(size_t)j + 1]; ++e) {
        const long long p = next[(size_t)row_idx[e]]++;
        ci[(size_t)p] = j; perm[(size_t)p] = e;
      }
  }
  // ---- device
  Scratch sc;
  double* v64 = sc.take<double>((size_t)nnz);
  long long* dperm = sc.take<long long>((size_t)nnz);
  double* sq = sc.take<double>((size_t)m);
  hipError_t e = sc.error();
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream);
  };
  up(vs.side[SIDE_G].sp_ptr, cp.data(), cp.size() * sizeof(long long));
  up(vs.side[SIDE_F].sp_ptr, rp.data(), rp.size() * sizeof(long long));
  up(vs.side[SIDE_G].sp_idx, row_idx, (size_t)nnz * sizeof(int));
  up(vs.side[SIDE_F].sp_idx, ci.data(), ci.size() * sizeof(int));
  up(v64, values, (size_t)nnz * sizeof(double));
  up(dperm, perm.data(), perm.size() * sizeof(long long));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(csc_normalise_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, h->stream, vs.side[SIDE_G].sp_ptr, v64, m, pre_processed ? 0 : 1,
                       vs.side[SIDE_G].sp_val, sq);
    if (nnz > 0)
      hipLaunchKernelGGL(csr_gather_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, h->stream, dperm, vs.side[SIDE_G].sp_val, nnz, vs.side[SIDE_F].sp_val);
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, h->stream, sq, m, vs.xnorm2);
    e = hipGetLastError();
  }
  e = plan_and_commit(h, vs, rp, cp, nnz, e);      // (synchronises: the host vectors go out of scope)
  if (e != hipSuccess) return h->fail_hip("set_view_csc", e);
  vs.empty_rows = vs.empty_cols = 0; vs.empty_mask.clear();
  return RESNMTF_OK;
}

int resnmtf_view_storage(resnmtf_handle* h, int v, int* is_sparse, long long* nnz, long long* nnz_capacity) {
  if (int rc = check_view(h, v)) return rc;
  const ViewState& vs = h->views[v];
  if (is_sparse) *is_sparse = vs.sparse ? 1 : 0;
  if (nnz) *nnz = vs.sparse ? vs.nnz : 0;
  if (nnz_capacity) *nnz_capacity = vs.sparse ? vs.nnz_cap : -1;
  return RESNMTF_OK;
}

// ---- view data without a host round trip (the k sweep re-uses one upload, the shuffles of
// spurious-bicluster removal are drawn on the device).  Every entry that fills a view of `dst` from a view of `src` --
// copy, shuffle and sub-sample, dense and sparse, and the count of a sparse sub-sample -- is refused by check_view_pair
// and starts its device work with begin_view_route.
namespace {
struct PairNeeds {
  const char* what;          // the entry's name: it heads every message
  bool sparse;               // the entry works on sparse views (else on dense ones) ...
  const char* other_entry;   // ... and this is what the message for a view of the other kind says in brackets
  bool same_shape;           // copy and shuffle; a sub-sample's shape is that of its index lists
  bool holds_source;         // the destination's nnz capacity must hold the source's stored entries
  bool has_dst = true;       // false: resnmtf_subsample_count_sparse, the source half alone (messages go to `dst`)
};
// The checks, in one order for every entry: destination view index, source handle NULL, source view index, destination
// kind, source kind, destination owned, source owned, source uploaded, shape, device, capacity.
int check_view_pair(resnmtf_handle* dst, int v, const resnmtf_handle* src, int v_src, const PairNeeds& need) {
  if (!dst) return RESNMTF_ERR_INVALID;
  if (need.has_dst)
    if (int rc = check_view(dst, v)) return rc;
  const std::string w = std::string(need.what) + ": ";
  const std::string other = std::string(need.sparse ? "dense (" : "sparse (") + need.other_entry + ")";
  if (!src) return dst->fail(RESNMTF_ERR_INVALID, w + "the source handle is NULL");
  if (v_src < 0 || v_src >= src->V) return dst->fail(RESNMTF_ERR_INVALID, w + "bad source view");
  const ViewState* a = need.has_dst ? &dst->views[v] : nullptr;
  const ViewState& b = src->views[v_src];
  if (a && a->sparse != need.sparse) return dst->fail(RESNMTF_ERR_INVALID, w + "the destination view is " + other);
  if (b.sparse != need.sparse) return dst->fail(RESNMTF_ERR_INVALID, w + "the source view is " + other);
  if (a && !a->owned) return dst->fail(RESNMTF_ERR_STATE, w + "the destination view is not owned");
  if (!b.owned) return dst->fail(RESNMTF_ERR_STATE, w + "the source view is not owned");
  if (!b.has_x) return dst->fail(RESNMTF_ERR_STATE, w + "the source view has not been uploaded");
  if (a && need.same_shape && (a->n != b.n || a->m != b.m)) return dst->fail(RESNMTF_ERR_INVALID, w + "views differ in shape");
  if (dst->opt.device_id != src->opt.device_id) return dst->fail(RESNMTF_ERR_INVALID, w + "handles live on different devices");
  if (a && need.holds_source && b.nnz > a->nnz_cap)
    return dst->fail(RESNMTF_ERR_INVALID, w + "the source holds " + std::to_string(b.nnz) + " stored entries, above the destination's nnz capacity " +
                     std::to_string(a->nnz_cap));
  return RESNMTF_OK;
}
// What follows every successful check: the device, the source's stream drained (its view is complete), then dst's own.
int begin_view_route(resnmtf_handle* dst, const resnmtf_handle* src) {
  HIP_TRY(dst, hipSetDevice(dst->opt.device_id));
  HIP_TRY(dst, hipStreamSynchronize(src->stream));
  return sync_both(dst);
}
constexpr PairNeeds kCopyView{"copy_view", false, "resnmtf_copy_view_sparse copies sparse views", true, false};
constexpr PairNeeds kShuffleView{"shuffle_view", false, "resnmtf_shuffle_view_sparse shuffles sparse views", true, false};
constexpr PairNeeds kSubsampleView{"subsample_view", false, "resnmtf_subsample_view_sparse sub-samples sparse views", false, false};
constexpr PairNeeds kCopySparse{"copy_view_sparse", true, "resnmtf_copy_view copies dense views", true, true};
constexpr PairNeeds kShuffleSparse{"shuffle_view_sparse", true, "resnmtf_shuffle_view shuffles dense views", true, true};
constexpr PairNeeds kSubsampleSparse{"subsample_view_sparse", true, "resnmtf_subsample_view sub-samples dense views", false, false};
constexpr PairNeeds kSubsampleCount{"subsample_count_sparse", true, "resnmtf_subsample_view sub-samples dense views", false, false, false};

// The index lists of a sub-sample, checked on the host: in range and, `distinct`, free of repeats (the reference samples
// without replacement, and a repeated row has no inverse map: the sparse route; the dense gather takes repeats).  `h`
// takes the refusal's text.
int check_sample_lists(resnmtf_handle* h, const char* what, const ViewState& b, int n_dst, const int* rows, int m_dst, const int* cols,
                       bool distinct) {
  const std::string w = std::string(what) + ": ";
  std::vector<unsigned char> seen((size_t)std::max(b.n, b.m), 0);
  for (int i = 0; i < n_dst; ++i) {
    if (rows[i] < 0 || rows[i] >= b.n) return h->fail(RESNMTF_ERR_INVALID, w + "row index out of range");
    if (distinct && seen[(size_t)rows[i]])
      return h->fail(RESNMTF_ERR_INVALID, w + "row index " + std::to_string(rows[i]) + " occurs twice (sub-samples are drawn without replacement)");
    seen[(size_t)rows[i]] = 1;
  }
  std::fill(seen.begin(), seen.end(), 0);
  for (int j = 0; j < m_dst; ++j) {
    if (cols[j] < 0 || cols[j] >= b.m) return h->fail(RESNMTF_ERR_INVALID, w + "column index out of range");
    if (distinct && seen[(size_t)cols[j]])
      return h->fail(RESNMTF_ERR_INVALID, w + "column index " + std::to_string(cols[j]) + " occurs twice (sub-samples are drawn without replacement)");
    seen[(size_t)cols[j]] = 1;
  }
  return RESNMTF_OK;
}
}  // namespace

int resnmtf_copy_view(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src) {
  if (int rc = check_view_pair(dst, v, src, v_src, kCopyView)) return rc;
  ViewState& a = dst->views[v];
  const ViewState& b = src->views[v_src];
  dst->resume_ok = false;
  if (int rc = begin_view_route(dst, src)) return rc;
  // same shape and options decide the same pitches; guard anyway
  if (a.side[SIDE_G].ldx != b.side[SIDE_G].ldx || a.side[SIDE_F].ldx != b.side[SIDE_F].ldx) return dst->fail(RESNMTF_ERR_INVALID, "views differ in device layout (no_pitch_pad)");
  HIP_TRY(dst, hipMemcpyAsync(a.side[SIDE_G].X, b.side[SIDE_G].X, a.side[SIDE_G].x_floats * sizeof(float), hipMemcpyDeviceToDevice, dst->stream));
  HIP_TRY(dst, hipMemcpyAsync(a.side[SIDE_F].X, b.side[SIDE_F].X, a.side[SIDE_F].x_floats * sizeof(float), hipMemcpyDeviceToDevice, dst->stream));
  HIP_TRY(dst, hipMemcpyAsync(a.xnorm2, b.xnorm2, sizeof(double), hipMemcpyDeviceToDevice, dst->stream));
  HIP_TRY(dst, hipStreamSynchronize(dst->stream));
  a.has_x = true;
  if (a.half_capable) return build_half_images(dst, a);
  return RESNMTF_OK;
}

int resnmtf_shuffle_view(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, unsigned long long seed, int normalise) {
  if (int rc = check_view_pair(dst, v, src, v_src, kShuffleView)) return rc;
  const ViewState& b = src->views[v_src];
  if (int rc = begin_view_route(dst, src)) return rc;
  const ShuffleSrc sh{b.side[SIDE_G].X, b.side[SIDE_G].ldx, seed, nullptr, nullptr};
  return upload_view(dst, v, nullptr, normalise != 0, nullptr, &sh);
}

int resnmtf_subsample_view(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, const int* rows, const int* cols) {
  if (int rc = check_view_pair(dst, v, src, v_src, kSubsampleView)) return rc;
  if (!rows || !cols) return dst->fail(RESNMTF_ERR_INVALID, "subsample_view: rows / cols are NULL");
  const ViewState& a = dst->views[v];
  const ViewState& b = src->views[v_src];
  if (int rc = check_sample_lists(dst, "subsample_view", b, a.n, rows, a.m, cols, false)) return rc;
  if (int rc = begin_view_route(dst, src)) return rc;
  Scratch sc;
  int* idx = sc.take<int>((size_t)a.n + a.m);
  hipError_t e = sc.error();
  if (e == hipSuccess) e = hipMemcpy(idx, rows, (size_t)a.n * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(idx + a.n, cols, (size_t)a.m * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) return dst->fail_hip("subsample_view", e);
  const ShuffleSrc sh{b.side[SIDE_G].X, b.side[SIDE_G].ldx, 0ull, idx, idx + a.n};
  return upload_view(dst, v, nullptr, false, nullptr, &sh);      // sub-samples are NOT re-normalised (Appendix B11)
}

// ---- sparse views built on the device from (destination position, value) pairs: the shuffle and the sub-sample
namespace {
// The transient device memory of one such build: five 8-byte arrays of nnz (two key buffers, the fp64 values, two payload
// buffers) + rocPRIM's histograms, the per-column squares and the line masks, all taken from the caller's Scratch.
struct SparseBuild {
  unsigned long long* key[2];
  long long* pay[3];             // 8-byte payloads: the fp64 values (first sort), CSC positions (second)
  double* sq;
  unsigned char* line_mask;
};
SparseBuild take_sparse_build(Scratch& sc, long long nnz, int n, int m) {
  SparseBuild sb{};
  for (auto& p : sb.key) p = sc.take<unsigned long long>((size_t)nnz);
  for (auto& p : sb.pay) p = sc.take<long long>((size_t)nnz);
  sb.sq = sc.take<double>((size_t)m);
  sb.line_mask = sc.take<unsigned char>((size_t)n + m + 2 * sizeof(int) + 8);
  return sb;
}

// The tail resnmtf_shuffle_view_sparse and resnmtf_subsample_view_sparse share.  On entry sb.key[0][0 .. nnz) holds the
// column-major destination position c' n + r' of every entry (distinct, any order) and sb.pay[0] its value as fp64, both
// enqueued on dst's stream; `e` is the status so far.  The entries sorted by position ARE the CSC (the keys are distinct,
// so the sorted order is unique and every correct sort gives the same bits); sorted by r' m + c' they are the CSR; then
// the masks of the lines without an entry > 0, the values (normalised or as they are), data_norms, the plan of the
// passes and the view's state.  nnz = 0: zero pointers, every line empty, nothing of size zero launched.
// The seam of resnmtf_set_view_sparse_device (the shuffle and the sub-sample leave both at their defaults): `presorted`
// -- the keys already ascend strictly, the first sort is skipped and key[0] / pay[0] go straight to the CSC stage;
// `check_sorted` -- called with the sorted keys between the first sort and the first store into the view's own arrays,
// a non-zero return (the refusal, already recorded on dst) ends the build there.
int finish_sparse_build(resnmtf_handle* dst, ViewState& a, Scratch& sc, const SparseBuild& sb, long long nnz, int normalise, hipError_t e,
                        const char* what, bool presorted = false,
                        const std::function<int(const unsigned long long*)>& check_sorted = nullptr) {
  const int n = a.n, m = a.m;
  hipStream_t st = dst->stream;
  std::vector<long long> cp((size_t)m + 1, 0), rp((size_t)n + 1, 0);
  std::vector<int> line_counts(2, 0);
  a.empty_rows = a.empty_cols = 0; a.empty_mask.assign((size_t)n + m, 1);
  const double* v64 = reinterpret_cast<const double*>(sb.pay[0]);
  if (e == hipSuccess && nnz == 0) {          // every line empty: zero pointers, nothing of size zero launched
    e = hipMemsetAsync(a.side[SIDE_G].sp_ptr, 0, ((size_t)m + 1) * sizeof(long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(a.side[SIDE_F].sp_ptr, 0, ((size_t)n + 1) * sizeof(long long), st);
    line_counts[0] = n; line_counts[1] = m;
  }
  if (e == hipSuccess && nnz > 0) {
    const unsigned grid = (unsigned)((nnz + 255) / 256);
    const unsigned long long count = (unsigned long long)n * m;
    unsigned int end_bit = 1;                           // the bits of n m: every key is < count
    while (end_bit < 64 && ((count - 1) >> end_bit) != 0) ++end_bit;
    // ---- the CSC: the entries sorted by destination position
    rocprim::double_buffer<unsigned long long> kb(sb.key[0], sb.key[1]);
    rocprim::double_buffer<double> vb(reinterpret_cast<double*>(sb.pay[0]), reinterpret_cast<double*>(sb.pay[1]));
    size_t tmp_bytes = 0, tmp_bytes2 = 0;
    e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, vb, (size_t)nnz, 0u, end_bit, st);
    rocprim::double_buffer<unsigned long long> kb2(sb.key[0], sb.key[1]);
    rocprim::double_buffer<long long> pb(sb.pay[1], sb.pay[2]);
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, tmp_bytes2, kb2, pb, (size_t)nnz, 0u, end_bit, st);
    tmp_bytes = std::max<size_t>(std::max(tmp_bytes, tmp_bytes2), 8);
    void* tmp = e == hipSuccess ? sc.take<char>(tmp_bytes) : nullptr;
    if (e == hipSuccess) e = sc.error();
    if (e == hipSuccess && !presorted) e = rocprim::radix_sort_pairs(tmp, tmp_bytes, kb, vb, (size_t)nnz, 0u, end_bit, st);
    if (e == hipSuccess && check_sorted)
      if (int rc = check_sorted(kb.current())) return rc;
    if (e == hipSuccess) {
      v64 = vb.current();
      hipLaunchKernelGGL(sorted_lines_kernel, dim3(grid), dim3(256), 0, st, kb.current(), nnz, (unsigned long long)n, m, a.side[SIDE_G].sp_ptr, a.side[SIDE_G].sp_idx);
      // ---- the CSR: the CSC positions sorted by r' m + c' (the values stay where the first sort left them)
      kb2 = rocprim::double_buffer<unsigned long long>(kb.alternate(), kb.current());
      pb = rocprim::double_buffer<long long>(reinterpret_cast<long long*>(vb.alternate()), sb.pay[2]);
      hipLaunchKernelGGL(sparse_shuffle_csr_keys_kernel, dim3(grid), dim3(256), 0, st, kb.current(), nnz, n, m, kb2.current(), pb.current());
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(tmp, tmp_bytes, kb2, pb, (size_t)nnz, 0u, end_bit, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(sorted_lines_kernel, dim3(grid), dim3(256), 0, st, kb2.current(), nnz, (unsigned long long)m, n, a.side[SIDE_F].sp_ptr, a.side[SIDE_F].sp_idx);
      int* counts = reinterpret_cast<int*>(sb.line_mask + (((size_t)n + m + 7) / 8) * 8);
      e = hipMemsetAsync(counts, 0, 2 * sizeof(int), st);
      hipLaunchKernelGGL(sparse_empty_lines_kernel, dim3(ceil_div(n + m, 256)), dim3(256), 0, st, a.side[SIDE_G].sp_ptr, a.side[SIDE_F].sp_ptr, pb.current(), v64, n, m,
                         sb.line_mask, counts);
      if (e == hipSuccess) e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(a.empty_mask.data(), sb.line_mask, (size_t)n + m, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(line_counts.data(), counts, 2 * sizeof(int), hipMemcpyDeviceToHost, st);
    }
    // ---- values: matrix_normalisation (fp64, ascending entry order) or the copy, data_norms, the CSR values
    if (e == hipSuccess) {
      hipLaunchKernelGGL(csc_normalise_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, a.side[SIDE_G].sp_ptr, v64, m, normalise ? 1 : 0, a.side[SIDE_G].sp_val, sb.sq);
      hipLaunchKernelGGL(csr_gather_kernel, dim3(grid), dim3(256), 0, st, pb.current(), a.side[SIDE_G].sp_val, nnz, a.side[SIDE_F].sp_val);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(cp.data(), a.side[SIDE_G].sp_ptr, cp.size() * sizeof(long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(rp.data(), a.side[SIDE_F].sp_ptr, rp.size() * sizeof(long long), hipMemcpyDeviceToHost, st);
  } else if (e == hipSuccess) {
    hipLaunchKernelGGL(csc_normalise_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, a.side[SIDE_G].sp_ptr, v64, m, 0, a.side[SIDE_G].sp_val, sb.sq);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, st, sb.sq, m, a.xnorm2);
    e = hipGetLastError();
  }
  e = plan_and_commit(dst, a, rp, cp, nnz, e);                   // the line pointers are on the host: plan the passes
  if (e != hipSuccess) { a.empty_mask.clear(); return dst->fail_hip(what, e); }
  a.empty_rows = line_counts[0]; a.empty_cols = line_counts[1];
  return RESNMTF_OK;
}

// The counting half of a sub-sample of source view b (resnmtf_sparse_subsample.hip.inc steps 1 and 2) on stream st: the
// lists and the inverse row map on the device, the kept entries per destination column and their exclusive scan cp, the
// total back on the host.  Transient: 4 (n' + m' + n_src) + 16 (m' + 1) bytes + rocPRIM's scan storage, from `sc`.
struct SubsampleMap {
  int* idx = nullptr;            // rows [n_dst], then cols [m_dst]
  int* inv_row = nullptr;        // [n_src]
  long long* cp = nullptr;       // [m_dst + 1]
};
hipError_t subsample_count(hipStream_t st, Scratch& sc, const ViewState& b, int n_dst, const int* rows, int m_dst, const int* cols,
                           SubsampleMap& sm, long long* total) {
  *total = 0;
  if (b.nnz == 0) return hipSuccess;                      // nothing stored, nothing kept: no launch
  sm.idx = sc.take<int>((size_t)n_dst + m_dst);
  sm.inv_row = sc.take<int>((size_t)b.n);
  long long* counts = sc.take<long long>((size_t)m_dst + 1);
  sm.cp = sc.take<long long>((size_t)m_dst + 1);
  hipError_t e = sc.error();
  if (e == hipSuccess) e = hipMemcpyAsync(sm.idx, rows, (size_t)n_dst * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(sm.idx + n_dst, cols, (size_t)m_dst * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(sm.inv_row, 0xFF, (size_t)b.n * sizeof(int), st);       // every row -1: not kept
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sparse_subsample_inverse_kernel, dim3(ceil_div(n_dst, 256)), dim3(256), 0, st, sm.idx, n_dst, sm.inv_row);
  hipLaunchKernelGGL(sparse_subsample_count_kernel, dim3(ceil_div(m_dst + 1, 4)), dim3(256), 0, st, b.side[SIDE_G].sp_ptr, b.side[SIDE_G].sp_idx,
                     sm.idx + n_dst, m_dst, sm.inv_row, counts);
  e = hipGetLastError();
  size_t tmp_bytes = 0;
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, counts, sm.cp, 0LL, (size_t)m_dst + 1, rocprim::plus<long long>(), st);
  void* tmp = e == hipSuccess ? sc.take<char>(std::max<size_t>(tmp_bytes, 8)) : nullptr;
  if (e == hipSuccess) e = sc.error();
  if (e == hipSuccess) e = rocprim::exclusive_scan(tmp, tmp_bytes, counts, sm.cp, 0LL, (size_t)m_dst + 1, rocprim::plus<long long>(), st);
  if (e == hipSuccess) e = hipMemcpyAsync(total, sm.cp + m_dst, sizeof(long long), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}
}  // namespace

// shuffle_view (R/obtain_bicl.r:11-22) of a sparse view into a sparse view: the dense path's draw (feistel_perm, same seed)
// of the densified source, built from the stored entries alone (resnmtf_sparse_shuffle.hip.inc).  Transient device memory:
// SparseBuild's 40 bytes per stored entry.
int resnmtf_shuffle_view_sparse(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, unsigned long long seed, int normalise) {
  if (int rc = check_view_pair(dst, v, src, v_src, kShuffleSparse)) return rc;
  ViewState& a = dst->views[v];
  const ViewState& b = src->views[v_src];
  const int n = a.n, m = a.m;
  const long long nnz = b.nnz;
  dst->resume_ok = false;
  if (int rc = begin_view_route(dst, src)) return rc;
  Scratch sc;
  const SparseBuild sb = take_sparse_build(sc, nnz, n, m);
  hipError_t e = sc.error();
  if (e == hipSuccess && nnz > 0) {
    hipLaunchKernelGGL(sparse_shuffle_keys_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, dst->stream, b.side[SIDE_G].sp_ptr, b.side[SIDE_G].sp_idx,
                       b.side[SIDE_G].sp_val, nnz, n, m, seed, sb.key[0], reinterpret_cast<double*>(sb.pay[0]));
    e = hipGetLastError();
  }
  return finish_sparse_build(dst, a, sc, sb, nnz, normalise, e, "shuffle_view_sparse");
}

// The number of stored entries of X[rows, cols] of a sparse view (stored zeros count); nothing is built.
int resnmtf_subsample_count_sparse(resnmtf_handle* src, int v_src, int n_rows, const int* rows, int n_cols, const int* cols, long long* nnz) {
  if (int rc = check_view_pair(src, -1, src, v_src, kSubsampleCount)) return rc;
  if (!rows || !cols || !nnz) return src->fail(RESNMTF_ERR_INVALID, "subsample_count_sparse: rows / cols / nnz is NULL");
  if (n_rows < 0 || n_cols < 0) return src->fail(RESNMTF_ERR_INVALID, "subsample_count_sparse: negative index count");
  const ViewState& b = src->views[v_src];
  if (int rc = check_sample_lists(src, "subsample_count_sparse", b, n_rows, rows, n_cols, cols, true)) return rc;
  *nnz = 0;
  if (n_rows == 0 || n_cols == 0) return RESNMTF_OK;
  if (int rc = begin_view_route(src, src)) return rc;
  Scratch sc;
  SubsampleMap sm;
  const hipError_t e = subsample_count(src->stream, sc, b, n_rows, rows, n_cols, cols, sm, nnz);
  if (e != hipSuccess) return src->fail_hip("subsample_count_sparse", e);
  return RESNMTF_OK;
}

// data[[i]][row_samples[[i]], col_samples[[i]]] (R/stability_analysis.r:124, :184, :232, :238) of a sparse view into a
// sparse view: the values as stored (f32, not re-normalised: SURVEY B11), stored zeros kept.  The view is bit for bit
// resnmtf_set_view_csc(pre_processed = 1) of the same sub-sample of the source's read-back.  Transient device memory:
// SparseBuild's 40 bytes per kept entry + SubsampleMap.
int resnmtf_subsample_view_sparse(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, const int* rows, const int* cols) {
  if (int rc = check_view_pair(dst, v, src, v_src, kSubsampleSparse)) return rc;
  if (!rows || !cols) return dst->fail(RESNMTF_ERR_INVALID, "subsample_view_sparse: rows / cols are NULL");
  ViewState& a = dst->views[v];
  const ViewState& b = src->views[v_src];
  if (int rc = check_sample_lists(dst, "subsample_view_sparse", b, a.n, rows, a.m, cols, true)) return rc;
  if (int rc = begin_view_route(dst, src)) return rc;
  Scratch sc;
  SubsampleMap sm;
  long long nnz = 0;
  hipError_t e = subsample_count(dst->stream, sc, b, a.n, rows, a.m, cols, sm, &nnz);
  if (e != hipSuccess) return dst->fail_hip("subsample_view_sparse", e);
  if (nnz > a.nnz_cap)               // (the destination is still what it was)
    return dst->fail(RESNMTF_ERR_INVALID, "subsample_view_sparse: the sub-sample holds " + std::to_string(nnz) +
                     " stored entries, above the destination's nnz capacity " + std::to_string(a.nnz_cap));
  dst->resume_ok = false;
  const SparseBuild sb = take_sparse_build(sc, nnz, a.n, a.m);
  e = sc.error();
  if (e == hipSuccess && nnz > 0) {
    hipLaunchKernelGGL(sparse_subsample_emit_kernel, dim3(ceil_div(a.m, 4)), dim3(256), 0, dst->stream, b.side[SIDE_G].sp_ptr, b.side[SIDE_G].sp_idx,
                       b.side[SIDE_G].sp_val, sm.idx + a.n, a.n, a.m, sm.inv_row, sm.cp, sb.key[0], reinterpret_cast<double*>(sb.pay[0]));
    e = hipGetLastError();
  }
  return finish_sparse_build(dst, a, sc, sb, nnz, 0, e, "subsample_view_sparse");
}

// ---- what resnmtf_set_view_sparse_device and resnmtf_sparse_device_canonical (the fp64 path) share:
// the launches of the device checks and the text of a failure word
extern "C++" {
namespace {
void spdv_launch_ptr_check(hipStream_t st, bool i64, const void* ptr, int lines, long long nnz, unsigned long long* flags) {
  if (i64) hipLaunchKernelGGL(sparse_device_ptr_check_kernel<true>, dim3(ceil_div(lines + 1, 256)), dim3(256), 0, st, ptr, lines, nnz, flags);
  else hipLaunchKernelGGL(sparse_device_ptr_check_kernel<false>, dim3(ceil_div(lines + 1, 256)), dim3(256), 0, st, ptr, lines, nnz, flags);
}
// nnz >= 1
void spdv_launch_entries(hipStream_t st, int layout, bool i64, int dtype, const void* a0, const void* a1, const void* values, long long nnz,
                         int n, int m, unsigned long long* key, double* val, unsigned char* col_pos, unsigned long long* flags) {
  const dim3 grid((unsigned)((nnz + 255) / 256));
  pick_int<RESNMTF_SPARSE_CSC, RESNMTF_SPARSE_CSR, RESNMTF_SPARSE_COO>(layout, [&](auto lay) {
    pick_bools([&](auto wide) {
      pick_int<RESNMTF_DTYPE_F64, RESNMTF_DTYPE_F32, RESNMTF_DTYPE_F16, RESNMTF_DTYPE_BF16>(dtype, [&](auto dt) {
        hipLaunchKernelGGL((sparse_device_entries_kernel<decltype(lay)::value, decltype(wide)::value, decltype(dt)::value>), grid, dim3(256), 0, st,
                           a0, a1, values, nnz, n, m, key, val, col_pos, flags);
      });
    }, i64);
  });
}
// word = kind << 56 | the lowest offending line, entry or sorted position; dup_key: the sorted key there (SPDV_DUPLICATE)
std::string spdv_refusal_text(unsigned long long word, bool csc, long long nnz, int n, unsigned long long dup_key) {
  const char* pname = csc ? "col_ptr" : "row_ptr";
  const char* lname = csc ? "column" : "row";
  const unsigned long long kind = word >> 56;
  const std::string num = std::to_string((long long)(word & ((1ull << 56) - 1ull)));
  switch (kind) {
    case SPDV_PTR_FIRST: return std::string(pname) + "[0] must be 0 (0-based " + (csc ? "CSC)" : "CSR)");
    case SPDV_PTR_MONOTONE: return std::string(pname) + " is not monotone (" + lname + " " + num + ")";
    case SPDV_PTR_LAST: return std::string(pname) + "[" + num + "] must equal nnz = " + std::to_string(nnz);
    case SPDV_ROW_RANGE: return "row index out of range (entry " + num + ")";
    case SPDV_COL_RANGE: return "column index out of range (entry " + num + ")";
    case SPDV_NON_FINITE: return "non-finite entry (entry " + num + ")";
    case SPDV_NEGATIVE:
      return "negative entry (entry " + num +
             "): make_non_neg (R/utils.r:20-27) shifts a whole column by its minimum, which would turn every implicit zero of a "
             "sparse view positive -- shift the data on the host and upload it dense";
    case SPDV_DUPLICATE:
      return "position (row " + std::to_string(dup_key % (unsigned long long)n) + ", column " + std::to_string(dup_key / (unsigned long long)n) +
             ") is stored twice: coalesce the entries first (nothing is summed)";
    default:
      return "column " + num + " is all zero: matrix_normalisation (R/utils.r:86-88) would divide it by zero (a NaN column in the reference)";
  }
}
}  // namespace
}  // extern "C++"

// A sparse view from CSC / CSR / COO arrays in the caller's device memory (resnmtf_sparse_device_view.hip.inc, DESIGN.md
// section 16): checked on the device, turned into (position, value) pairs and built by finish_sparse_build.  Transient
// device memory: SparseBuild's 40 bytes per entry + m flag bytes + the two flag words.
int resnmtf_set_view_sparse_device(resnmtf_handle* h, int v, int layout, const void* ptr_or_rows, const void* idx_or_cols, int index_type,
                                   const void* values, int dtype, long long nnz, int pre_processed, void* stream) {
  const char* what = "set_view_sparse_device";
  const std::string w = std::string(what) + ": ";
  if (int rc = check_view(h, v)) return rc;
  ViewState& vs = h->views[v];
  if (!vs.sparse) return h->fail(RESNMTF_ERR_INVALID, "the view is dense: upload it with resnmtf_set_view / resnmtf_set_view_raw / resnmtf_set_view_device");
  if (!vs.owned) return h->fail(RESNMTF_ERR_STATE, w + "a view this handle does not own");
  if (layout != RESNMTF_SPARSE_CSC && layout != RESNMTF_SPARSE_CSR && layout != RESNMTF_SPARSE_COO)
    return h->fail(RESNMTF_ERR_INVALID, w + "unknown layout: one of RESNMTF_SPARSE_CSC / _CSR / _COO");
  if (index_type != RESNMTF_INDEX_I32 && index_type != RESNMTF_INDEX_I64)
    return h->fail(RESNMTF_ERR_INVALID, w + "unknown index type: RESNMTF_INDEX_I32 or _I64");
  if (dtype != RESNMTF_DTYPE_F64 && dtype != RESNMTF_DTYPE_F32 && dtype != RESNMTF_DTYPE_F16 && dtype != RESNMTF_DTYPE_BF16)
    return h->fail(RESNMTF_ERR_INVALID, w + "unknown dtype: one of RESNMTF_DTYPE_F64 / _F32 / _F16 / _BF16");
  if (nnz < 0) return h->fail(RESNMTF_ERR_INVALID, w + "nnz is negative");
  if (nnz > vs.nnz_cap)
    return h->fail(RESNMTF_ERR_INVALID, w + "nnz = " + std::to_string(nnz) + " exceeds the view's nnz capacity " + std::to_string(vs.nnz_cap));
  const bool coo = layout == RESNMTF_SPARSE_COO, csc = layout == RESNMTF_SPARSE_CSC;
  if ((!ptr_or_rows && !(coo && nnz == 0)) || ((!idx_or_cols || !values) && nnz > 0))
    return h->fail(RESNMTF_ERR_INVALID, w + "ptr_or_rows / idx_or_cols / values is NULL");
  for (const void* p : {ptr_or_rows, idx_or_cols, values})
    if (p && !on_handle_device(h, p))
      return h->fail(RESNMTF_ERR_INVALID, w + "an array is not device memory of the handle's device (host data: resnmtf_set_view_csc)");
  const int n = vs.n, m = vs.m, lines = csc ? m : n;
  const bool i64 = index_type == RESNMTF_INDEX_I64;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  hipStream_t st = h->stream;
  Scratch sc;
  unsigned long long* flags = sc.take<unsigned long long>(2);      // the failure word, "CSC rows not ascending"
  unsigned char* col_pos = pre_processed ? nullptr : sc.take<unsigned char>((size_t)m);
  if (sc.error() != hipSuccess) return h->fail_hip("hipMalloc set_view_sparse_device flags", sc.error());
  unsigned long long host_flags[2] = {kSpdvNone, 0ull};
  // the flags as they are on the device after everything enqueued so far; the refusal, if the word holds one
  auto verdict = [&](const unsigned long long* sorted_keys) -> int {
    hipError_t e = hipMemcpyAsync(host_flags, flags, sizeof(host_flags), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return h->fail_hip(what, e);
    if (host_flags[0] == kSpdvNone) return RESNMTF_OK;
    unsigned long long k = 0;                 // a duplicate is named by its position: the sorted key there
    if (host_flags[0] >> 56 == SPDV_DUPLICATE) {
      e = hipMemcpy(&k, sorted_keys + (host_flags[0] & ((1ull << 56) - 1ull)), sizeof(k), hipMemcpyDeviceToHost);
      if (e != hipSuccess) return h->fail_hip(what, e);
    }
    return h->fail(RESNMTF_ERR_INVALID, spdv_refusal_text(host_flags[0], csc, nnz, n, k));
  };
  hipError_t e = wait_for_caller(h, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(flags, host_flags, sizeof(host_flags), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && col_pos) e = hipMemsetAsync(col_pos, 0, (size_t)m, st);
  if (e != hipSuccess) return h->fail_hip(what, e);
  // ---- the line pointers, judged before any kernel bounds a search by them
  if (!coo) {
    spdv_launch_ptr_check(st, i64, ptr_or_rows, lines, nnz, flags);
    HIP_TRY(h, hipGetLastError());
    if (int rc = verdict(nullptr)) return rc;
  }
  if (nnz == 0 && !pre_processed)
    return h->fail(RESNMTF_ERR_INVALID, "column 0 is all zero: matrix_normalisation (R/utils.r:86-88) would divide it by zero (a NaN column in the reference)");
  // ---- the entries: checks, keys, values
  const SparseBuild sb = take_sparse_build(sc, nnz, n, m);
  if (sc.error() != hipSuccess) return h->fail_hip("hipMalloc set_view_sparse_device build", sc.error());
  if (nnz > 0) {
    spdv_launch_entries(st, layout, i64, dtype, ptr_or_rows, idx_or_cols, values, nnz, n, m, sb.key[0], reinterpret_cast<double*>(sb.pay[0]), col_pos, flags);
    if (col_pos) hipLaunchKernelGGL(sparse_device_columns_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, col_pos, m, flags);
    HIP_TRY(h, hipGetLastError());
    if (int rc = verdict(nullptr)) return rc;
  }
  // ---- the build.  A refusal at the duplicates stage comes before anything is stored into the view's arrays: what
  // finish_sparse_build has done to the empty-line state by then is put back.
  const bool presorted = csc && host_flags[1] == 0ull;
  const int empty_rows = vs.empty_rows, empty_cols = vs.empty_cols;
  std::vector<unsigned char> empty_mask = vs.empty_mask;
  h->resume_ok = false;
  std::function<int(const unsigned long long*)> duplicates;
  if (!presorted && nnz > 1)
    duplicates = [&](const unsigned long long* sorted_keys) -> int {
      hipLaunchKernelGGL(sparse_device_duplicates_kernel, dim3((unsigned)((nnz + 254) / 256)), dim3(256), 0, st, sorted_keys, nnz, flags);
      HIP_TRY(h, hipGetLastError());
      return verdict(sorted_keys);
    };
  const int rc = finish_sparse_build(h, vs, sc, sb, nnz, pre_processed ? 0 : 1, hipSuccess, what, presorted, duplicates);
  if (rc != RESNMTF_OK) { vs.empty_rows = empty_rows; vs.empty_cols = empty_cols; vs.empty_mask = std::move(empty_mask); return rc; }
  vs.empty_rows = vs.empty_cols = 0; vs.empty_mask.clear();      // (as after resnmtf_set_view_csc: not device-drawn data)
  return RESNMTF_OK;
}

// resnmtf_copy_view for sparse views: both pointer arrays, both index arrays, both value arrays and data_norms device to
// device.  The block lists and nsplit depend on KP (spmm_groups_host), and k may differ between the handles (the k sweep
// copies from a k = 2 base), so the 8 (n + m + 2) bytes of line pointers are read back and the passes planned again.
int resnmtf_copy_view_sparse(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src) {
  if (int rc = check_view_pair(dst, v, src, v_src, kCopySparse)) return rc;
  ViewState& a = dst->views[v];
  const ViewState& b = src->views[v_src];
  if (&a == &b) return RESNMTF_OK;
  const int n = a.n, m = a.m;
  const long long nnz = b.nnz;
  dst->resume_ok = false;
  if (int rc = begin_view_route(dst, src)) return rc;
  hipStream_t st = dst->stream;
  std::vector<long long> cp((size_t)m + 1, 0), rp((size_t)n + 1, 0);
  hipError_t e = hipSuccess;
  auto copy = [&](void* to, const void* from, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, st);
  };
  copy(a.side[SIDE_G].sp_ptr, b.side[SIDE_G].sp_ptr, cp.size() * sizeof(long long));
  copy(a.side[SIDE_F].sp_ptr, b.side[SIDE_F].sp_ptr, rp.size() * sizeof(long long));
  copy(a.side[SIDE_G].sp_idx, b.side[SIDE_G].sp_idx, (size_t)nnz * sizeof(int));
  copy(a.side[SIDE_F].sp_idx, b.side[SIDE_F].sp_idx, (size_t)nnz * sizeof(int));
  copy(a.side[SIDE_G].sp_val, b.side[SIDE_G].sp_val, (size_t)nnz * sizeof(float));
  copy(a.side[SIDE_F].sp_val, b.side[SIDE_F].sp_val, (size_t)nnz * sizeof(float));
  copy(a.xnorm2, b.xnorm2, sizeof(double));
  if (e == hipSuccess) e = hipMemcpyAsync(cp.data(), b.side[SIDE_G].sp_ptr, cp.size() * sizeof(long long), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(rp.data(), b.side[SIDE_F].sp_ptr, rp.size() * sizeof(long long), hipMemcpyDeviceToHost, st);
  e = plan_and_commit(dst, a, rp, cp, nnz, e);                  // the line pointers are on the host: plan the passes
  if (e != hipSuccess) { a.has_x = false; return dst->fail_hip("copy_view_sparse", e); }   // (the arrays may be partly overwritten)
  a.empty_rows = a.empty_cols = 0; a.empty_mask.clear();      // (as after resnmtf_set_view_csc: not device-drawn data)
  return RESNMTF_OK;
}

int resnmtf_view_empty_lines(resnmtf_handle* h, int v, int* n_empty_rows, int* n_empty_cols, unsigned char* row_mask,
                             unsigned char* col_mask) {
  if (int rc = check_view(h, v)) return rc;
  const ViewState& vs = h->views[v];
  if (n_empty_rows) *n_empty_rows = vs.empty_rows;
  if (n_empty_cols) *n_empty_cols = vs.empty_cols;
  const bool have = vs.empty_mask.size() == (size_t)vs.n + vs.m;
  if (row_mask) for (int r = 0; r < vs.n; ++r) row_mask[r] = have ? vs.empty_mask[(size_t)r] : 0;
  if (col_mask) for (int c = 0; c < vs.m; ++c) col_mask[c] = have ? vs.empty_mask[(size_t)vs.n + c] : 0;
  return RESNMTF_OK;
}

int resnmtf_get_view(resnmtf_handle* h, int v, double* x) {
  if (int rc = check_view(h, v)) return rc;
  if (!x) return h->fail(RESNMTF_ERR_INVALID, "x is NULL");
  const ViewState& vs = h->views[v];
  if (vs.sparse) return h->fail(RESNMTF_ERR_INVALID, "get_view of a sparse view is not supported (it would densify it)");
  if (!vs.owned || !vs.has_x) return h->fail(RESNMTF_ERR_STATE, "no data on this handle for the view");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  std::vector<float> t(vs.side[SIDE_F].x_floats);                  // Xt32(c, r) = X[r][c], tile-major over r
  HIP_TRY(h, hipMemcpy(t.data(), vs.side[SIDE_F].X, t.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int c = 0; c < vs.m; ++c)
    for (int r = 0; r < vs.n; ++r) x[(size_t)c * vs.n + r] = (double)t[xidx(c, r, vs.side[SIDE_F].ldx)];
  return RESNMTF_OK;
}

// the device CSC copy of a sparse view back on the host (sizes from resnmtf_view_storage); never densifies
int resnmtf_get_view_csc(resnmtf_handle* h, int v, long long* col_ptr, int* row_idx, double* values) {
  if (int rc = check_view(h, v)) return rc;
  const ViewState& vs = h->views[v];
  if (!vs.sparse) return h->fail(RESNMTF_ERR_INVALID, "get_view_csc of a dense view: read it with resnmtf_get_view");
  if (!vs.owned || !vs.has_x) return h->fail(RESNMTF_ERR_STATE, "no data on this handle for the view");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  if (col_ptr) HIP_TRY(h, hipMemcpy(col_ptr, vs.side[SIDE_G].sp_ptr, ((size_t)vs.m + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (row_idx && vs.nnz > 0) HIP_TRY(h, hipMemcpy(row_idx, vs.side[SIDE_G].sp_idx, (size_t)vs.nnz * sizeof(int), hipMemcpyDeviceToHost));
  if (values && vs.nnz > 0) {
    std::vector<float> t((size_t)vs.nnz);
    HIP_TRY(h, hipMemcpy(t.data(), vs.side[SIDE_G].sp_val, t.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < t.size(); ++e) values[e] = (double)t[e];
  }
  return RESNMTF_OK;
}

// The dense view into caller-owned device memory (resnmtf_view_readback.hip.inc): the image
// resnmtf_get_view downloads, copied by one kernel, ordered with `stream` as resnmtf_finalise_device orders its copies; no
// transient memory.
int resnmtf_get_view_device(resnmtf_handle* h, int v, void* out, int dtype, long long row_stride, long long col_stride, void* stream) {
  const std::string w = "get_view_device: ";
  if (int rc = check_view(h, v)) return rc;
  if (!out) return h->fail(RESNMTF_ERR_INVALID, w + "out is NULL");
  if (dtype == RESNMTF_DTYPE_F16 || dtype == RESNMTF_DTYPE_BF16)
    return h->fail(RESNMTF_ERR_INVALID, w + "a 16-bit output would narrow the stored f32 values, which is not a copy: RESNMTF_DTYPE_F64 or _F32");
  if (dtype != RESNMTF_DTYPE_F64 && dtype != RESNMTF_DTYPE_F32) return h->fail(RESNMTF_ERR_INVALID, w + "unknown dtype: RESNMTF_DTYPE_F64 or _F32");
  const ViewState& vs = h->views[v];
  if (vs.sparse) return h->fail(RESNMTF_ERR_INVALID, w + "the view is sparse (it would densify it): read it with resnmtf_get_view_sparse_device");
  if (!vs.owned || !vs.has_x) return h->fail(RESNMTF_ERR_STATE, "no data on this handle for the view");
  const int n = vs.n, m = vs.m;
  if ((n > 1 && row_stride <= 0) || (m > 1 && col_stride <= 0))
    return h->fail(RESNMTF_ERR_INVALID, w + "a stride along an extent above 1 must be positive");
  if (n > 1 && m > 1) {      // no two elements on one address: the smaller stride's whole extent fits below the larger stride
    const bool rows_inner = row_stride <= col_stride;
    const long long a = rows_inner ? row_stride : col_stride, b = rows_inner ? col_stride : row_stride;
    const long long e = rows_inner ? n : m;
    if (a * (e - 1) >= b) return h->fail(RESNMTF_ERR_INVALID, w + "the strides make two elements share an address");
  }
  if (!on_handle_device(h, out))
    return h->fail(RESNMTF_ERR_INVALID, w + "out is not device memory of the handle's device (host buffers: resnmtf_get_view)");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  HIP_TRY(h, wait_for_caller(h, stream));
  const dim3 grid((unsigned)ceil_div(n, 32) * (unsigned)ceil_div(m, 32));
  const bool along_c = col_stride < row_stride;      // neighbouring lanes write along the smaller stride
  pick_bools([&](auto f64, auto ac) {
    using OUT = std::conditional_t<decltype(f64)::value, double, float>;
    hipLaunchKernelGGL((view_readback_kernel<OUT, decltype(ac)::value>), grid, dim3(256), 0, h->stream, (const float*)vs.side[SIDE_F].X,
                       vs.side[SIDE_F].ldx, n, m, static_cast<OUT*>(out), row_stride, col_stride);
  }, dtype == RESNMTF_DTYPE_F64, along_c);
  hipError_t e = hipGetLastError();
  // (the handle's stream is drained before the call returns: whatever the caller enqueues afterwards comes after the writes)
  const hipError_t es = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return h->fail_hip("get_view_device", e);
  return RESNMTF_OK;
}

// The sparse view into caller-owned device memory, the mirror of resnmtf_set_view_sparse_device:
// the CSC copy, the CSR copy, or the CSR copy with its row pointers expanded to a row index per entry (COO).  A kept type
// is a device-to-device copy, a widened or narrowed one a conversion kernel; no transient memory.
int resnmtf_get_view_sparse_device(resnmtf_handle* h, int v, int layout, void* ptr_or_rows, void* idx_or_cols, int index_type, void* values,
                                   int dtype, void* stream) {
  const std::string w = "get_view_sparse_device: ";
  if (int rc = check_view(h, v)) return rc;
  const ViewState& vs = h->views[v];
  if (!vs.sparse) return h->fail(RESNMTF_ERR_INVALID, w + "the view is dense: read it with resnmtf_get_view_device");
  if (layout != RESNMTF_SPARSE_CSC && layout != RESNMTF_SPARSE_CSR && layout != RESNMTF_SPARSE_COO)
    return h->fail(RESNMTF_ERR_INVALID, w + "unknown layout: one of RESNMTF_SPARSE_CSC / _CSR / _COO");
  if (index_type != RESNMTF_INDEX_I32 && index_type != RESNMTF_INDEX_I64)
    return h->fail(RESNMTF_ERR_INVALID, w + "unknown index type: RESNMTF_INDEX_I32 or _I64");
  if (dtype == RESNMTF_DTYPE_F16 || dtype == RESNMTF_DTYPE_BF16)
    return h->fail(RESNMTF_ERR_INVALID, w + "a 16-bit output would narrow the stored f32 values, which is not a copy: RESNMTF_DTYPE_F64 or _F32");
  if (dtype != RESNMTF_DTYPE_F64 && dtype != RESNMTF_DTYPE_F32) return h->fail(RESNMTF_ERR_INVALID, w + "unknown dtype: RESNMTF_DTYPE_F64 or _F32");
  if (!vs.owned || !vs.has_x) return h->fail(RESNMTF_ERR_STATE, "no data on this handle for the view");
  const long long nnz = vs.nnz;
  const bool i64 = index_type == RESNMTF_INDEX_I64;
  if (!i64 && nnz > 2147483647LL)
    return h->fail(RESNMTF_ERR_INVALID, w + "nnz = " + std::to_string(nnz) + " does not fit RESNMTF_INDEX_I32: ask for RESNMTF_INDEX_I64");
  for (const void* p : {(const void*)ptr_or_rows, (const void*)idx_or_cols, (const void*)values})
    if (p && !on_handle_device(h, p))
      return h->fail(RESNMTF_ERR_INVALID, w + "an array is not device memory of the handle's device (host buffers: resnmtf_get_view_csc)");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  HIP_TRY(h, wait_for_caller(h, stream));
  hipStream_t st = h->stream;
  const bool csc = layout == RESNMTF_SPARSE_CSC, coo = layout == RESNMTF_SPARSE_COO;
  const Side& sd = vs.side[csc ? SIDE_G : SIDE_F];      // the CSC copy walks the columns (SIDE_G), the CSR copy the rows
  const long long lines = sd.len;
  auto blocks = [](long long count) { return dim3((unsigned)((count + 255) / 256)); };
  hipError_t e = hipSuccess;
  if (ptr_or_rows && coo && nnz > 0) {
    if (i64) hipLaunchKernelGGL(readback_expand_rows_kernel<long long>, blocks(nnz), dim3(256), 0, st, (const long long*)sd.sp_ptr, vs.n, nnz, static_cast<long long*>(ptr_or_rows));
    else hipLaunchKernelGGL(readback_expand_rows_kernel<int>, blocks(nnz), dim3(256), 0, st, (const long long*)sd.sp_ptr, vs.n, nnz, static_cast<int*>(ptr_or_rows));
  } else if (ptr_or_rows && !coo) {
    if (i64) e = hipMemcpyAsync(ptr_or_rows, sd.sp_ptr, (size_t)(lines + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
    else hipLaunchKernelGGL((readback_convert_kernel<long long, int>), blocks(lines + 1), dim3(256), 0, st, (const long long*)sd.sp_ptr, lines + 1, static_cast<int*>(ptr_or_rows));
  }
  if (e == hipSuccess && idx_or_cols && nnz > 0) {
    if (!i64) e = hipMemcpyAsync(idx_or_cols, sd.sp_idx, (size_t)nnz * sizeof(int), hipMemcpyDeviceToDevice, st);
    else hipLaunchKernelGGL((readback_convert_kernel<int, long long>), blocks(nnz), dim3(256), 0, st, (const int*)sd.sp_idx, nnz, static_cast<long long*>(idx_or_cols));
  }
  if (e == hipSuccess && values && nnz > 0) {
    if (dtype == RESNMTF_DTYPE_F32) e = hipMemcpyAsync(values, sd.sp_val, (size_t)nnz * sizeof(float), hipMemcpyDeviceToDevice, st);
    else hipLaunchKernelGGL((readback_convert_kernel<float, double>), blocks(nnz), dim3(256), 0, st, (const float*)sd.sp_val, nnz, static_cast<double*>(values));
  }
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return h->fail_hip("get_view_sparse_device", e);
  return RESNMTF_OK;
}

namespace {
// The tail of both factor routes (resnmtf_set_factors, resnmtf_set_factors_device) for an owned view, once W of both sides
// and both lm vectors are on their way on the handle's stream: the zeroed operand images, T32 and counters, then the f32 /
// bf16 operand copies of the new factors.
hipError_t enqueue_factor_images(resnmtf_handle* h, ViewState& vs) {
  hipError_t e = hipMemsetAsync(vs.side[SIDE_F].W32, 0, (size_t)vs.n_pad * 64 * sizeof(float), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(vs.side[SIDE_G].W32, 0, (size_t)vs.m_pad * 64 * sizeof(float), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(vs.T32, 0, (size_t)vs.m_pad * 64 * sizeof(float), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(vs.side[SIDE_F].cnt, 0, 4 * sizeof(int), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(vs.side[SIDE_G].cnt, 0, 4 * sizeof(int), h->stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(factor_to_f32_kernel, dim3(ceil_div(vs.n * vs.k, 256)), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n,
                     vs.k, vs.side[SIDE_F].W32, vs.kk_mode == 0 ? vs.KP : 64, vs.NT, vs.half ? 1 : 0, vs.side[SIDE_F].Wk);
  hipLaunchKernelGGL(factor_to_f32_kernel, dim3(ceil_div(vs.m * vs.k, 256)), dim3(256), 0, h->stream, vs.side[SIDE_G].W, vs.m,
                     vs.k, vs.side[SIDE_G].W32, vs.kk_mode == 0 ? vs.KP : 64, vs.NT, vs.half ? 1 : 0, vs.side[SIDE_G].Wk);
  return hipGetLastError();
}
}  // namespace

int resnmtf_set_factors(resnmtf_handle* h, int v, const double* F, const double* S, const double* G,
                        const double* lambda, const double* mu) {
  if (int rc = check_view(h, v)) return rc;
  if (!F || !S || !G) return h->fail(RESNMTF_ERR_INVALID, "F, S and G are required");
  ViewState& vs = h->views[v];
  h->resume_ok = false;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  std::vector<double> f, s, g;
  to_row_major(F, vs.n, vs.k, f);
  to_row_major(S, vs.k, vs.k, s);
  to_row_major(G, vs.m, vs.k, g);
  HIP_TRY(h, hipMemcpyAsync(vs.side[SIDE_F].W, f.data(), f.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(vs.S, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(vs.side[SIDE_G].W, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  std::vector<double> lam(vs.k, 0.0), muv(vs.k, 0.0);
  if (vs.owned) {
    // explicit-init branch: lambda = colSums(F), mu = colSums(G) (R/update_steps.r:55-56)
    for (int j = 0; j < vs.k; ++j) {
      if (lambda) lam[j] = lambda[j];
      else { double t = 0.0; for (int i = 0; i < vs.n; ++i) t += F[(size_t)j * vs.n + i]; lam[j] = t; }
      if (mu) muv[j] = mu[j];
      else { double t = 0.0; for (int i = 0; i < vs.m; ++i) t += G[(size_t)j * vs.m + i]; muv[j] = t; }
    }
    HIP_TRY(h, hipMemcpyAsync(vs.side[SIDE_F].lm, lam.data(), lam.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(vs.side[SIDE_G].lm, muv.data(), muv.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, enqueue_factor_images(h, vs));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // host vectors go out of scope
  vs.has_factors = true;
  return RESNMTF_OK;
}

// The device route: the kernels of resnmtf_device_factors.hip.inc widen the caller's matrices
// straight into W / S / lm once the handle's stream has waited for the caller's; no host copy, no transient memory.
int resnmtf_set_factors_device(resnmtf_handle* h, int v, const resnmtf_device_matrix* F, const resnmtf_device_matrix* S,
                               const resnmtf_device_matrix* G, const resnmtf_device_matrix* lambda,
                               const resnmtf_device_matrix* mu, void* stream) {
  if (int rc = check_view(h, v)) return rc;
  if (!F || !S || !G || !F->ptr || !S->ptr || !G->ptr) return h->fail(RESNMTF_ERR_INVALID, "F, S and G are required");
  if ((lambda && !lambda->ptr) || (mu && !mu->ptr)) return h->fail(RESNMTF_ERR_INVALID, "lambda / mu: the matrix has a NULL ptr (pass NULL for colSums)");
  ViewState& vs = h->views[v];
  for (const resnmtf_device_matrix* a : {F, S, G, lambda, mu}) {
    if (!a) continue;
    if (a->dtype != RESNMTF_DTYPE_F64 && a->dtype != RESNMTF_DTYPE_F32 && a->dtype != RESNMTF_DTYPE_F16 && a->dtype != RESNMTF_DTYPE_BF16)
      return h->fail(RESNMTF_ERR_INVALID, "unknown dtype: one of RESNMTF_DTYPE_F64 / _F32 / _F16 / _BF16");
    if (a->row_stride < 0 || a->col_stride < 0) return h->fail(RESNMTF_ERR_INVALID, "negative strides are not supported");
  }
  for (const resnmtf_device_matrix* a : {F, S, G, lambda, mu})
    if (a && !on_handle_device(h, a->ptr))
      return h->fail(RESNMTF_ERR_INVALID, "a factor is not device memory of the handle's device (host factors: resnmtf_set_factors)");
  if ((lambda || mu) && !vs.owned) return h->fail(RESNMTF_ERR_STATE, "lambda/mu only exist on the owning handle");
  h->resume_ok = false;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  HIP_TRY(h, wait_for_caller(h, stream));
  // rows x cols of `a` into the row-major fp64 dst; a column-major source (row stride 1) goes through the LDS transpose
  auto widen = [&](const resnmtf_device_matrix* a, int rows, int cols, double* dst) {
    pick_int<RESNMTF_DTYPE_F64, RESNMTF_DTYPE_F32, RESNMTF_DTYPE_F16, RESNMTF_DTYPE_BF16>(a->dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      if (a->row_stride == 1 && a->col_stride != 1)
        hipLaunchKernelGGL(device_factor_transpose_kernel<DT>, dim3(ceil_div(rows, 32) * ceil_div(cols, 32)), dim3(256), 0, h->stream, a->ptr,
                           a->row_stride, a->col_stride, rows, cols, dst, (long long)cols, 1LL);
      else
        hipLaunchKernelGGL(device_factor_copy_kernel<DT>, dim3((unsigned)(((size_t)rows * cols + 255) / 256)), dim3(256), 0, h->stream, a->ptr,
                           a->row_stride, a->col_stride, rows, cols, dst);
    });
  };
  widen(F, vs.n, vs.k, vs.side[SIDE_F].W);
  widen(S, vs.k, vs.k, vs.S);
  widen(G, vs.m, vs.k, vs.side[SIDE_G].W);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && vs.owned) {
    // explicit-init branch: lambda = colSums(F), mu = colSums(G) (R/update_steps.r:55-56), in the host route's order
    if (lambda) widen(lambda, vs.k, 1, vs.side[SIDE_F].lm);
    if (mu) widen(mu, vs.k, 1, vs.side[SIDE_G].lm);
    if (!lambda || !mu)
      hipLaunchKernelGGL(device_factor_colsum_kernel, dim3(2), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n,
                         lambda ? (double*)nullptr : vs.side[SIDE_F].lm, vs.side[SIDE_G].W, vs.m, mu ? (double*)nullptr : vs.side[SIDE_G].lm, vs.k);
    e = hipGetLastError();
    if (e == hipSuccess) e = enqueue_factor_images(h, vs);
  }
  const hipError_t es = hipStreamSynchronize(h->stream);   // the sources may be freed on return
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return h->fail_hip("set_factors_device", e);
  vs.has_factors = true;
  return RESNMTF_OK;
}

// ---------------------------------------------------------------------------------------------
// resnmtf_init_svd -- init_mats_inner (R/update_steps.r:78-125) for one view, SURVEY 8(f1).
// Randomized subspace iteration (L = 16 ceil((k + 8) / 16) <= 64 columns): the two big products per
// iteration are the streaming-pass kernels; CholeskyQR2 orthonormalisation and the final L x L
// symmetric eigenproblem are fp64, their L x L factorisations on the host.
// ---------------------------------------------------------------------------------------------
// (cholesky_upper, invert_upper and jacobi_eigen, the L x L factorisations: resnmtf_small_linalg.h, shared with the fp64 unit)
namespace {
// the work arrays of the SVD initialisation, taken from the Scratch of the route (Pn / Pm: the view's own slabs or temporaries)
struct InitScratch {
  double *Yn = nullptr, *Yn2 = nullptr, *Zm = nullptr, *Zm2 = nullptr, *gpart = nullptr, *gram = nullptr, *M = nullptr;
  float *Pn = nullptr, *Pm = nullptr;
};
constexpr int kGramBlocks = 256;

// gram = Y^T Y (L x L) on the host
int ts_gram_host(resnmtf_handle* h, InitScratch& sc, const double* Y, int len, int L, std::vector<double>& C) {
  const int rpb = round_up(ceil_div(len, kGramBlocks), 16), nblk = ceil_div(len, rpb);
  hipLaunchKernelGGL(ts_gram_kernel, dim3(nblk), dim3(256), 0, h->stream, Y, len, L, rpb, sc.gpart);
  hipLaunchKernelGGL(reduce_records_kernel, dim3(ceil_div(L * L, 256)), dim3(256), 0, h->stream, sc.gpart, nblk, L * L, sc.gram);
  C.resize((size_t)L * L);
  HIP_TRY(h, hipMemcpyAsync(C.data(), sc.gram, C.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return RESNMTF_OK;
}
int ts_apply(resnmtf_handle* h, InitScratch& sc, const double* Y, int len, int L, const std::vector<double>& M,
             double* Q, float* W32, int nt) {
  HIP_TRY(h, hipMemcpyAsync(sc.M, M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(ts_apply_kernel, dim3(ceil_div(len * L, 256)), dim3(256), 0, h->stream, Y, len, L, sc.M, Q, W32, 64, nt);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));       // M (host vector) may go out of scope
  return RESNMTF_OK;
}
// CholeskyQR2: Y (in `a`) -> orthonormal columns (back in `a`, `b` is scratch) + f32 operand copy.
// Rank cut (kRankCut): a sketch of a view whose rank is below L has columns that depend on the others -- exactly so when
// rows of X repeat or are zero, since equal rows of X give bitwise equal rows of every product.  Their pivots are the
// ridge alone in round 0 and rounding noise in round 1, where dividing by them gave a basis that was neither orthonormal
// nor in the range of X (or no factorisation at all).  Such a column is zeroed instead, in both rounds: it stays zero
// through the products that follow and ends as a zero singular value with zero vectors.  A pivot above the cut takes
// the same arithmetic as before, so a sketch of full rank keeps its bits.
constexpr double kRankCut = 2e-14;      // times trace(C): twice the ridge of round 0, 1e4 x the rounding of a pivot
int orthonormalise(resnmtf_handle* h, InitScratch& sc, double* a, double* b, int len, int L, float* W32, int nt) {
  std::vector<double> C, R, Ri;
  for (int round = 0; round < 2; ++round) {
    double* src = round == 0 ? a : b;
    double* dst = round == 0 ? b : a;
    if (int rc = ts_gram_host(h, sc, src, len, L, C)) return rc;
    double tr = 0.0;
    for (int i = 0; i < L; ++i) tr += C[(size_t)i * L + i];
    if (round == 0)              // tiny ridge: sketches of nearly rank-deficient data stay factorable
      for (int i = 0; i < L; ++i) C[(size_t)i * L + i] += 1e-14 * tr;
    const int kept = cholesky_upper(C, L, kRankCut * tr, R);
    if (kept < 0) return h->fail(RESNMTF_ERR_INVALID, "init_svd: the view holds entries that are not finite");
    if (kept == 0) return h->fail(RESNMTF_ERR_INVALID, "init_svd: the view is all zero");
    invert_upper(R, L, Ri);
    if (int rc = ts_apply(h, sc, src, len, L, Ri, dst, round == 1 ? W32 : nullptr, nt)) return rc;
  }
  return RESNMTF_OK;
}
}  // namespace

namespace {
// the signed basis resnmtf_init_svd_basis hands back (all four pointers set, or no BasisOut at all)
struct BasisOut { double *U, *V, *d; int* n_d; };

// R/update_steps.r:93-115 on the k leading triplets: U (n x ldu), V (m x ldv) row-major, d descending.
// Column-major outputs go through resnmtf_set_factors.
int finish_init(resnmtf_handle* h, int v, const std::vector<double>& U, int ldu, const std::vector<double>& V, int ldv,
                const std::vector<double>& d, double sigma, std::mt19937_64& gen, double* singular_values, const BasisOut* basis) {
  const ViewState& vs = h->views[v];
  const int n = vs.n, m = vs.m, k = vs.k;
  if (basis) {
    for (int j = 0; j < k; ++j) {
      for (int i = 0; i < n; ++i) basis->U[(size_t)j * n + i] = U[(size_t)i * ldu + j];
      for (int i = 0; i < m; ++i) basis->V[(size_t)j * m + i] = V[(size_t)i * ldv + j];
    }
    for (size_t j = 0; j < d.size(); ++j) basis->d[j] = d[j];
    *basis->n_d = (int)d.size();
  }
  std::vector<double> F0((size_t)n * k), G0((size_t)m * k), S0((size_t)k * k, 0.0), cf(k, 0.0), cg(k, 0.0), lam(k, 0.0), muv(k, 0.0);
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i < n; ++i) { const double a = std::fabs(U[(size_t)i * ldu + j]); F0[(size_t)j * n + i] = a; cf[j] += a; }   // :93,:100
    for (int i = 0; i < m; ++i) { const double a = std::fabs(V[(size_t)i * ldv + j]); G0[(size_t)j * m + i] = a; cg[j] += a; }   // :94,:101
    // a zero vector (a triplet past the rank of X): svd() returns some unit vector there; the constant one stands in
    if (cf[j] == 0.0) { for (int i = 0; i < n; ++i) F0[(size_t)j * n + i] = 1.0 / std::sqrt((double)n); cf[j] = std::sqrt((double)n); }
    if (cg[j] == 0.0) { for (int i = 0; i < m; ++i) G0[(size_t)j * m + i] = 1.0 / std::sqrt((double)m); cg[j] = std::sqrt((double)m); }
  }
  std::normal_distribution<double> noise(0.0, std::sqrt(sigma));                    // mvrnorm(k, 0, sigma I), :96-99
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      double sv = (i == j ? std::fabs(d[j]) : 0.0);                                 // :95
      if (sigma > 0.0) sv += std::fabs(noise(gen));
      S0[(size_t)j * k + i] = sv * cf[j] * cg[j];                                   // :102-105 (column sweep)
    }
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i < n; ++i) { F0[(size_t)j * n + i] /= cf[j]; lam[j] += F0[(size_t)j * n + i]; }   // :106-109,:114
    for (int i = 0; i < m; ++i) { G0[(size_t)j * m + i] /= cg[j]; muv[j] += G0[(size_t)j * m + i]; }   // :110-113,:115
  }
  if (singular_values)
    for (int j = 0; j < k; ++j) singular_values[j] = d[j];
  return resnmtf_set_factors(h, v, F0.data(), S0.data(), G0.data(), lam.data(), muv.data());
}

// Thin views (min(n, m) smaller than the sketch): the exact SVD through the Gram matrix of the short
// side -- Y = X (m <= n) or X^T, C = Y^T Y (r x r, fp64, device), Jacobi on the host, the long-side
// vectors Y W Sigma^-1 on the device.  No random sketch, no iteration.
int init_svd_thin(resnmtf_handle* h, int v, double sigma, std::mt19937_64& gen, double* singular_values, const BasisOut* basis) {
  ViewState& vs = h->views[v];
  const int n = vs.n, m = vs.m;
  const bool tall = m <= n;                       // Y = X [n][m]  or  X^T [m][n]
  const int len = tall ? n : m, r = tall ? m : n;
  Scratch mem;
  InitScratch sc;
  sc.Yn = mem.take<double>((size_t)len * r); sc.Yn2 = mem.take<double>((size_t)len * r);
  sc.gpart = mem.take<double>((size_t)(kGramBlocks + 1) * r * r); sc.gram = mem.take<double>((size_t)r * r);
  sc.M = mem.take<double>((size_t)r * r);
  if (mem.error() != hipSuccess) return h->fail_hip("init_svd hipMalloc", mem.error());
  const int long_side = tall ? SIDE_F : SIDE_G;      // Y has one row per line of the long side
  const Side& lines = vs.side[long_side];
  if (vs.sparse) {      // the short side from the CSR (Y = X) or the CSC (Y = X^T)
    HIP_TRY(h, hipMemsetAsync(sc.Yn, 0, (size_t)len * r * sizeof(double), h->stream));
    hipLaunchKernelGGL(sparse_widen_kernel, dim3(ceil_div(len, 256)), dim3(256), 0, h->stream, lines.sp_ptr, lines.sp_idx, lines.sp_val, len, r, sc.Yn);
  } else
    hipLaunchKernelGGL(widen_rows_kernel, dim3(ceil_div(len * r, 256)), dim3(256), 0, h->stream, vs.side[other(long_side)].X, vs.side[other(long_side)].ldx, len, r, sc.Yn);
  HIP_TRY(h, hipGetLastError());
  std::vector<double> C, W;
  if (int rc = ts_gram_host(h, sc, sc.Yn, len, r, C)) return rc;
  jacobi_eigen(C, r, W);
  std::vector<int> order(r);
  for (int i = 0; i < r; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return C[(size_t)a * r + a] > C[(size_t)b * r + b]; });
  std::vector<double> d(r), Ws((size_t)r * r), Wn((size_t)r * r);
  for (int j = 0; j < r; ++j) {
    const int src = order[j];
    d[j] = std::sqrt(std::max(C[(size_t)src * r + src], 0.0));
    for (int i = 0; i < r; ++i) {
      Ws[(size_t)i * r + j] = W[(size_t)i * r + src];
      Wn[(size_t)i * r + j] = d[j] > 0.0 ? W[(size_t)i * r + src] / d[j] : 0.0;
    }
  }
  if (int rc = ts_apply(h, sc, sc.Yn, len, r, Wn, sc.Yn2, nullptr, 1)) return rc;     // long-side vectors
  std::vector<double> Lg((size_t)len * r);
  HIP_TRY(h, hipMemcpyAsync(Lg.data(), sc.Yn2, Lg.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return tall ? finish_init(h, v, Lg, r, Ws, r, d, sigma, gen, singular_values, basis)
              : finish_init(h, v, Ws, r, Lg, r, d, sigma, gen, singular_values, basis);
}

int init_svd_impl(resnmtf_handle* h, int v, unsigned long long seed, double sigma, int n_power, double* singular_values,
                  const BasisOut* basis) {
  ViewState& vs = h->views[v];
  if (!vs.owned || !vs.has_x) return h->fail(RESNMTF_ERR_STATE, "init_svd needs an owned view with data (set_view first)");
  if (n_power < 1) n_power = 3;
  if (!(sigma >= 0.0)) return h->fail(RESNMTF_ERR_INVALID, "sigma must be >= 0");
  h->resume_ok = false;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  const int n = vs.n, m = vs.m, k = vs.k;
  const int L = std::min(64, 16 * ceil_div(k + 8, 16)), NTi = L / 16;
  std::mt19937_64 gen(seed);
  if (std::min(n, m) < L) return init_svd_thin(h, v, sigma, gen, singular_values, basis);
  Scratch mem;
  InitScratch sc;
  sc.Yn = mem.take<double>((size_t)n * L); sc.Yn2 = mem.take<double>((size_t)n * L);
  sc.Zm = mem.take<double>((size_t)m * L); sc.Zm2 = mem.take<double>((size_t)m * L);
  sc.gpart = mem.take<double>((size_t)(kGramBlocks + 1) * L * L); sc.gram = mem.take<double>((size_t)L * L);
  sc.M = mem.take<double>((size_t)L * L);
  if (mem.error() != hipSuccess) return h->fail_hip("init_svd hipMalloc", mem.error());
  // slabs: the view's own when the sketch is as wide as its KP, else temporaries
  if (L == vs.KP) { sc.Pn = vs.side[SIDE_F].P; sc.Pm = vs.side[SIDE_G].P; }
  else {
    sc.Pn = mem.take<float>((size_t)vs.side[SIDE_F].nsplit * vs.n_pad * L);
    sc.Pm = mem.take<float>((size_t)vs.side[SIDE_G].nsplit * vs.m_pad * L);
    if (mem.error() != hipSuccess) return h->fail_hip("init_svd hipMalloc slabs", mem.error());
  }
  PassArgs xg{}, xt{};
  xg.A = vs.side[SIDE_F].X; xg.lda = 64; xg.tile_stride = vs.side[SIDE_F].ldx; xg.ntiles = vs.n_pad / 64; xg.B = vs.side[SIDE_G].W32; xg.ldb = 64; xg.P = sc.Pn;
  xg.cols_pad = vs.n_pad; xg.rows_pad = vs.m_pad; xg.rows_per_split = vs.side[SIDE_F].rps; xg.nsplit = vs.side[SIDE_F].nsplit; xg.ctl = h->ctl;
  xt.A = vs.side[SIDE_G].X; xt.lda = 64; xt.tile_stride = vs.side[SIDE_G].ldx; xt.ntiles = vs.m_pad / 64; xt.B = vs.side[SIDE_F].W32; xt.ldb = 64; xt.P = sc.Pm;
  xt.cols_pad = vs.m_pad; xt.rows_pad = vs.n_pad; xt.rows_per_split = vs.side[SIDE_G].rps; xt.nsplit = vs.side[SIDE_G].nsplit; xt.ctl = h->ctl;

  // Omega: m x L standard normal (host generator: the reference's RNG is not reproducible anyway)
  std::normal_distribution<double> normal(0.0, 1.0);
  std::vector<double> omega((size_t)m * L);
  for (double& x : omega) x = normal(gen);
  HIP_TRY(h, hipMemcpyAsync(sc.Zm, omega.data(), omega.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(vs.side[SIDE_F].W32, 0, (size_t)vs.n_pad * 64 * sizeof(float), h->stream));
  HIP_TRY(h, hipMemsetAsync(vs.side[SIDE_G].W32, 0, (size_t)vs.m_pad * 64 * sizeof(float), h->stream));
  hipLaunchKernelGGL(factor_to_f32_kernel, dim3(ceil_div(m * L, 256)), dim3(256), 0, h->stream, sc.Zm, m, L, vs.side[SIDE_G].W32, 64, NTi, 0, (unsigned short*)nullptr);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  // sparse view: the same products from the CSR / CSC (spmm_kernel without a k x k job), the same slabs
  SpmmArgs sxg = spmm_args(vs, true), sxt = spmm_args(vs, false);
  sxg.B = vs.side[SIDE_G].W32; sxg.ldb = 64; sxg.P = sc.Pn; sxg.ctl = h->ctl;
  sxt.B = vs.side[SIDE_F].W32; sxt.ldb = 64; sxt.P = sc.Pm; sxt.ctl = h->ctl;
  auto product = [&](bool is_xg) {
    if (!vs.sparse) launch_pass_plain(h, is_xg ? xg : xt, NTi, is_xg);
    else launch_spmm(h, is_xg ? sxg : sxt, L, is_xg, KKFArgs{}, KKSArgs{});
  };
  for (int it = 0; it < n_power; ++it) {
    product(true);                                                                         // Y = X Z
    hipLaunchKernelGGL(slab_sum_kernel, dim3(ceil_div(n * L, 256)), dim3(256), 0, h->stream, sc.Pn, vs.side[SIDE_F].nsplit, vs.n_pad, L, n, sc.Yn);
    HIP_TRY(h, hipGetLastError());
    if (int rc = orthonormalise(h, sc, sc.Yn, sc.Yn2, n, L, vs.side[SIDE_F].W32, NTi)) return rc;          // Q (in Yn) + F32
    product(false);                                                                        // Z = X^T Q
    hipLaunchKernelGGL(slab_sum_kernel, dim3(ceil_div(m * L, 256)), dim3(256), 0, h->stream, sc.Pm, vs.side[SIDE_G].nsplit, vs.m_pad, L, m, sc.Zm);
    HIP_TRY(h, hipGetLastError());
    if (it + 1 < n_power)
      if (int rc = orthonormalise(h, sc, sc.Zm, sc.Zm2, m, L, vs.side[SIDE_G].W32, NTi)) return rc;
  }
  // Z = X^T Q = V Sigma Ut^T  ->  Z^T Z = Ut Sigma^2 Ut^T;  U = Q Ut,  V = Z Ut Sigma^-1
  std::vector<double> C, Ut;
  if (int rc = ts_gram_host(h, sc, sc.Zm, m, L, C)) return rc;
  jacobi_eigen(C, L, Ut);
  std::vector<int> order(L);
  for (int i = 0; i < L; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return C[(size_t)a * L + a] > C[(size_t)b * L + b]; });
  std::vector<double> d(L), Mu((size_t)L * L), Mv((size_t)L * L);
  for (int j = 0; j < L; ++j) {
    const int src = order[j];
    d[j] = std::sqrt(std::max(C[(size_t)src * L + src], 0.0));
    for (int i = 0; i < L; ++i) {
      Mu[(size_t)i * L + j] = Ut[(size_t)i * L + src];
      Mv[(size_t)i * L + j] = d[j] > 0.0 ? Ut[(size_t)i * L + src] / d[j] : 0.0;
    }
  }
  if (int rc = ts_apply(h, sc, sc.Yn, n, L, Mu, sc.Yn2, nullptr, NTi)) return rc;             // U (n x L)
  if (int rc = ts_apply(h, sc, sc.Zm, m, L, Mv, sc.Zm2, nullptr, NTi)) return rc;             // V (m x L)
  std::vector<double> U((size_t)n * L), V((size_t)m * L);
  HIP_TRY(h, hipMemcpyAsync(U.data(), sc.Yn2, U.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(V.data(), sc.Zm2, V.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return finish_init(h, v, U, L, V, L, d, sigma, gen, singular_values, basis);
}
}  // namespace

int resnmtf_init_svd(resnmtf_handle* h, int v, unsigned long long seed, double sigma, int n_power,
                     double* singular_values) {
  if (int rc = check_view(h, v)) return rc;
  return init_svd_impl(h, v, seed, sigma, n_power, singular_values, nullptr);
}

int resnmtf_init_svd_basis(resnmtf_handle* h, int v, unsigned long long seed, double sigma, int n_power,
                           double* singular_values, double* U, double* V, double* d, int* n_d) {
  if (int rc = check_view(h, v)) return rc;
  if (!U || !V || !d || !n_d) return h->fail(RESNMTF_ERR_INVALID, "init_svd_basis: U, V, d and n_d must not be NULL");
  const BasisOut basis{U, V, d, n_d};
  return init_svd_impl(h, v, seed, sigma, n_power, singular_values, &basis);
}

int resnmtf_set_restrictions(resnmtf_handle* h, const double* phi, const double* xi, const double* psi) {
  if (!h) return RESNMTF_ERR_INVALID;
  const size_t cnt = (size_t)h->V * h->V;
  const double* src[3] = {phi, xi, psi};
  std::vector<double>* dst[3] = {&h->phi, &h->xi, &h->psi};
  for (int t = 0; t < 3; ++t) {
    if (src[t]) {
      for (size_t e = 0; e < cnt; ++e)
        if (!(src[t][e] >= 0.0)) return h->fail(RESNMTF_ERR_INVALID, "restriction matrices must be non-negative (R/utils.r:343-355)");
      dst[t]->assign(src[t], src[t] + cnt);
    } else {
      dst[t]->assign(cnt, 0.0);
    }
  }
  h->prepared = false;
  h->resume_ok = false;
  return RESNMTF_OK;
}

static int set_shared(resnmtf_handle* h, int v, int w, int count, const int* idx_v, const int* idx_w, bool rows) {
  if (int rc = check_view(h, v)) return rc;
  if (int rc = check_view(h, w)) return rc;
  if (v == w) return h->fail(RESNMTF_ERR_INVALID, "shared map needs two different views");
  ViewState& vs = h->views[v];
  const ViewState& ws = h->views[w];
  const int s = rows ? SIDE_F : SIDE_G;
  SharedMap& mp = vs.side[s].map[w];
  const int len_v = vs.side[s].len, len_w = ws.side[s].len;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  h->prepared = false;
  h->resume_ok = false;
  if (count < 0) {           // NA
    mp.set = true; mp.count = -1;
    if (mp.dev) { (void)hipFree(mp.dev); mp.dev = nullptr; }
    return RESNMTF_OK;
  }
  if (count > 0 && (!idx_v || !idx_w)) return h->fail(RESNMTF_ERR_INVALID, "index arrays are NULL");
  std::vector<int> map((size_t)len_v, -1);
  for (int t = 0; t < count; ++t) {
    if (idx_v[t] < 0 || idx_v[t] >= len_v || idx_w[t] < 0 || idx_w[t] >= len_w)
      return h->fail(RESNMTF_ERR_INVALID, "shared index out of range");
    map[idx_v[t]] = idx_w[t];
  }
  if (!mp.dev) HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&mp.dev), (size_t)len_v * sizeof(int)));
  HIP_TRY(h, hipMemcpy(mp.dev, map.data(), (size_t)len_v * sizeof(int), hipMemcpyHostToDevice));
  mp.set = true; mp.count = count;
  mp.identity = true;
  for (int r = 0; r < len_v && mp.identity; ++r) mp.identity = map[r] == r;
  return RESNMTF_OK;
}

int resnmtf_set_shared_rows(resnmtf_handle* h, int v, int w, int count, const int* idx_v, const int* idx_w) {
  return set_shared(h, v, w, count, idx_v, idx_w, true);
}
int resnmtf_set_shared_cols(resnmtf_handle* h, int v, int w, int count, const int* idx_v, const int* idx_w) {
  return set_shared(h, v, w, count, idx_v, idx_w, false);
}

// ---- the chain builders.  What is the same for every chain of side s: the per-view fields (fill_chain_view) and the
// coupling table (fill_coupling); what differs is listed at each builder.
extern "C++" {      // (templates: ChainArgs<8> and WideChainArgs<8> share the field names)
// cmask / weight of view v from the couple list of its update: which views' running factors it reads, and how strongly
template <class Chain>
static void fill_coupling(const resnmtf_handle* h, int s, int v, const UpdateArgs& u, Chain& a) {
  for (int c = 0; c < u.n_couple; ++c)
    for (int w = 0; w < h->V; ++w)
      if (u.couple[c].W == h->views[w].side[s].W) { a.cmask[v] |= 1u << w; a.weight[v][w] = u.couple[c].weight; }
}
// W, U, Ma, Md, lm, sigma, n_other, the restricted bit and the couplings of view v, from the update arguments of its side s
template <class Chain>
static void fill_chain_view(const resnmtf_handle* h, int s, int v, Chain& a) {
  const UpdateArgs& u = h->views[v].side[s].arg;
  a.W[v] = u.W; a.U[v] = u.P; a.Ma[v] = u.Ma; a.Md[v] = u.Md; a.lm[v] = u.lm;
  a.sigma[v] = u.sigma;
  a.n_other[v] = (double)u.len;
  if (u.restricted) a.restricted |= 1u << v;
  fill_coupling(h, s, v, u, a);
}
}  // extern "C++"
static bool identity_coupled(const UpdateArgs& u) {      // a permuted shared map: rows of other workgroups
  for (int c = 0; c < u.n_couple; ++c)
    if (u.couple[c].map) return false;
  return true;
}

// RESNMTF_PHASE_F_ALL (s = SIDE_F) / RESNMTF_PHASE_G_ALL (SIDE_G; replicated G chain, R/update_steps.r:195-204) at k <= 16 in
// one f_chain_kernel launch: every view holds the inputs of that update here (owned, or a replica), hand-off mode A, equal
// lengths, k and blocking, every coupling through identity maps, at most 8 views.  Otherwise one launch per view.
// Where the two sides differ:          F                                   G
//   layout gate                        --                                  replicate_gs and not slice_chains
//   slabs per view (u.nsplit)          up to 4 raw split slabs             1 (the folded slab of the exchange block)
//   2-byte images (half)               allowed, but the same in all        not allowed
//                                      owned views (one kpack32)
//   owned views                        at most 4                           at most 2
static void build_chain(resnmtf_handle* h, int s) {
  h->chain_views[s] = 0;
  const int V = h->V;
  if (V < 2 || V > 8 || h->opt.no_f_chain) return;
  if (s == SIDE_G && (!h->opt.replicate_gs || h->sliced)) return;
  const int max_nsplit = s == SIDE_F ? 4 : 1, max_owned = s == SIDE_F ? 4 : 2;
  const ViewState& v0 = h->views[0];
  const Side& s0 = v0.side[s];
  int n_owned = 0, kpack = -1;
  for (int v = 0; v < V; ++v) {
    const ViewState& vs = h->views[v];
    const Side& sd = vs.side[s];
    if (!vs.owned && !sd.replica) return;
    if (s == SIDE_G && vs.half) return;
    if (vs.owned) {                                         // one operand-copy layout for all owned views
      if (kpack < 0) kpack = vs.half ? 1 : 0;
      else if (kpack != (vs.half ? 1 : 0)) return;
    }
    if (vs.KP != 16 || vs.kk_mode != 0 || sd.len != s0.len || vs.k != v0.k || sd.rpb != s0.rpb || sd.nblk != s0.nblk) return;
    if (sd.arg.nsplit > max_nsplit || sd.arg.cols_pad != s0.arg.cols_pad) return;     // raw split slabs the kernel keeps per view
    if (vs.owned && ++n_owned > max_owned) return;
    if (!identity_coupled(sd.arg)) return;
  }
  ChainArgs<8>& a = h->chain[s];
  a = ChainArgs<8>{};
  a.len = s0.len; a.k = v0.k; a.n_views = V; a.rows_per_block = s0.rpb;
  a.ctl = h->ctl;
  a.pstride = (size_t)s0.arg.cols_pad * 16;
  a.kpack32 = kpack > 0 ? 1 : 0;
  for (int v = 0; v < 8; ++v) a.emit_slot[v] = -1;
  for (int v = 0; v < V; ++v) {
    const ViewState& vs = h->views[v];
    const Side& sd = vs.side[s];
    if (vs.owned) {
      a.emit_slot[v] = a.n_emit;
      a.W32e[a.n_emit] = sd.W32; a.parte[a.n_emit] = sd.part;
      if (s == SIDE_G) a.T32e[a.n_emit] = vs.T32;
      ++a.n_emit;
    }
    fill_chain_view(h, s, v, a);
    a.nsplit[v] = sd.arg.nsplit;
  }
  h->chain_views[s] = V;
  h->chain_blocks[s] = s0.nblk;
}

// RESNMTF_PHASE_F_ALL / G_ALL in one launch at k = 32 / 64 (wide_chain_kernel): every view holds the inputs of the update
// here (owned or replica) as ONE folded slab (the exchange blocks of replicate_f / replicate_gs), equal lengths and k,
// every coupling through identity maps, at most one owned view, at most 8 views.  Otherwise one launch per view.
static void build_wide_chain(resnmtf_handle* h) {
  h->wchain_ok[0] = h->wchain_ok[1] = false;
  const int V = h->V;
  if (V < 2 || V > 8 || h->opt.no_f_chain) return;
  const ViewState& v0 = h->views[0];
  if (v0.KP < 32 || h->sliced) return;
  for (int g = 0; g < 2; ++g) {
    WideChainArgs<8>& a = h->wchain[g];
    a = WideChainArgs<8>{};
    a.own = -1;
    bool ok = true;
    int n_owned = 0;
    for (int v = 0; v < V && ok; ++v) {
      const ViewState& vs = h->views[v];
      const Side& sd = vs.side[g];
      const UpdateArgs& u = sd.arg;
      if (!vs.owned && !sd.replica) { ok = false; break; }
      if (vs.KP != v0.KP || vs.k != v0.k || sd.len != v0.side[g].len) { ok = false; break; }
      if (u.nsplit != 1 || u.P == nullptr) { ok = false; break; }            // the folded slab of an exchange block
      if (!identity_coupled(u)) ok = false;
      if (vs.owned) {
        if (++n_owned > 1) { ok = false; break; }
        a.own = v; a.W32 = sd.W32; a.Wk = sd.Wk; a.T32 = g == SIDE_F ? nullptr : vs.T32; a.ld32 = u.ld32;
        if (!a.W32 || !a.Wk || (g == SIDE_G && !a.T32)) { ok = false; break; }
      }
      fill_chain_view(h, g, v, a);
    }
    if (!ok) continue;
    a.len = v0.side[g].len; a.n_self = a.len; a.k = v0.k; a.n_views = V; a.ngroups = ceil_div(a.len, 32);
    a.ctl = h->ctl;
    // persistent workgroups: one per CU at k > 32 (157 KB of LDS at k = 64, 131 KB at 48), two at k = 32
    h->wchain_grid[g] = std::min(a.ngroups, h->n_cu * (v0.KP == 32 ? 2 : 1));
    h->wchain_ok[g] = true;
  }
}

// slice_chains: RESNMTF_PHASE_SLICE_F / _G -- the chain of every view on this rank's row (column) slice, one launch
// (wide_chain_kernel on the slice: inputs = the received rows of every view's product, outputs = the fp64 rows kept here and
// their f32 copies for the owners)
static int build_slice_chain(resnmtf_handle* h) {
  const int V = h->V, r = h->opt.slice_index;
  const ViewState& v0 = h->views[0];
  for (int g = 0; g < 2; ++g) {
    WideChainArgs<8>& a = h->schain[g];
    a = WideChainArgs<8>{};
    a.own = -1;
    const int per = h->sl_len[g], full = v0.side[g].len;
    const int begin = std::min(r * per, full), len = std::min(per, full - begin);
    for (int v = 0; v < V; ++v) {
      const ViewState& vs = h->views[v];
      if (!identity_coupled(vs.side[g].arg))
        return h->fail(RESNMTF_ERR_INVALID, "slice_chains: coupled views must share all their rows / columns in the same order (identity maps)");
      fill_chain_view(h, g, v, a);
      // this rank's slice: its rows of the factor, and the received chunk of view v's product (G: its Ma | Md ride behind it)
      a.W[v] = vs.side[g].W + (size_t)begin * vs.k;
      const char* chunk = h->p_recv[g] + (size_t)v * h->p_chunk[g];
      a.U[v] = reinterpret_cast<const float*>(chunk);
      if (g == SIDE_G) { a.Ma[v] = reinterpret_cast<const double*>(chunk + (size_t)per * vs.KP * sizeof(float)); a.Md[v] = a.Ma[v] + (size_t)vs.k * vs.k; }
      a.n_other[v] = (double)full;
    }
    a.O32 = h->w_send[g]; a.o32_stride = (unsigned)((size_t)per * v0.KP);
    if (h->opt.slice_p2p) {      // straight into the owner's receive slot for this rank's slice
      if (!h->p2p_ready) return h->fail(RESNMTF_ERR_STATE, "slice_p2p: import every rank's buffers first (resnmtf_p2p_import)");
      a.O32 = nullptr;
      for (int v = 0; v < V; ++v) a.O32v[v] = h->peers[(size_t)v].w_recv[g] + (size_t)r * per * v0.KP;
    }
    a.len = len; a.n_self = full; a.k = v0.k; a.n_views = V; a.ngroups = ceil_div(std::max(len, 0), 32);
    a.ctl = h->ctl;
    h->schain_grid[g] = std::min(a.ngroups, h->n_cu * (v0.KP <= 32 ? 2 : 1));
  }
  return RESNMTF_OK;
}

// the update arguments of side s of view v: R/update_steps.r:141-165 (F) / :180-207 (G), coupling table included
static int fill_update(resnmtf_handle* h, int v, int s) {
  const int V = h->V;
  ViewState& vs = h->views[v];
  Side& sd = vs.side[s];
  const std::vector<double>& coupling = s == SIDE_F ? h->phi : h->psi;
  UpdateArgs& u = sd.arg;
  u = UpdateArgs{};
  u.len = sd.len; u.k = vs.k; u.W = sd.W; u.W32 = sd.W32; u.Wk = sd.Wk; u.ld32 = vs.kk_mode == 0 ? vs.KP : 64; u.kpack32 = vs.half ? 1 : 0;
  u.P = sd.P; u.nsplit = sd.nsplit; u.cols_pad = sd.pad;
  if (sd.xsum) { u.P = sd.xsum; u.nsplit = 1; }      // replicate_f / replicate_gs: the folded slab of the exchange block
  u.Ma = sd.Ma; u.Md = sd.Md; u.lm = sd.lm; u.T32 = s == SIDE_G ? vs.T32 : nullptr; u.part = sd.part;
  if (!vs.owned && vs.NT >= 2) { u.W32 = nullptr; u.Wk = nullptr; u.T32 = nullptr; }   // only this view's passes (on its owner) read them
  u.rows_per_block = sd.rpb; u.ctl = h->ctl;
  double sigma = 0.0, whole = 0.0;
  for (int i = 0; i < V; ++i) sigma += coupling[(size_t)i + (size_t)v * V];       // sum(phi[, v]) (:150,:152) / sum(psi[, v]) (:195,:200)
  for (double x : coupling) whole += x;
  // the documented asymmetry: F restricts on its own column sum(phi[, v]); G branches on the WHOLE matrix sum(psi) (:190)
  u.restricted = ((s == SIDE_F ? sigma : whole) != 0.0) ? 1 : 0;
  u.sigma = sigma;
  u.n_couple = 0;
  for (int i = 0; i < V && u.restricted; ++i) {
    const double wgt = coupling[(size_t)i + (size_t)v * V];
    if (wgt == 0.0 || i == v) continue;                                            // utils.r:66
    const SharedMap& mp = sd.map[i];
    if (!mp.set || mp.count < 0) continue;                                         // NA: utils.r:70
    if (h->views[i].k != vs.k) return h->fail(RESNMTF_ERR_INVALID, s == SIDE_F ? "phi-coupled views need equal k" : "psi-coupled views need equal k");
    CoupleDesc& c = u.couple[u.n_couple++];
    c.W = h->views[i].side[s].W; c.map = mp.identity ? nullptr : mp.dev; c.weight = wgt; c.n_other = (double)h->views[i].side[s].len;
  }
  return RESNMTF_OK;
}
// the arguments of the pass that feeds side s of view v: it streams side s's image and multiplies by the OTHER side's factor
static void fill_pass(resnmtf_handle* h, int v, int s) {
  ViewState& vs = h->views[v];
  Side& sd = vs.side[s];
  const Side& b = vs.side[other(s)];
  PassArgs& a = sd.pass;
  a = PassArgs{};
  a.A = sd.X; a.lda = 64; a.tile_stride = sd.ldx; a.ntiles = sd.pad / 64; a.B = b.W32; a.Bk = b.Wk; a.ldb = vs.kk_mode == 0 ? vs.KP : 64; a.P = sd.P;
  a.cols_pad = sd.pad; a.rows_pad = b.pad; a.rows_per_split = sd.rps; a.nsplit = sd.nsplit;
  a.tw = sd.tw; a.ntg = ceil_div(a.ntiles, a.tw);
  a.A16 = sd.X16; a.tile_stride16 = sd.ld16;
  a.aux[0] = b.W32; a.naux = kAuxKinds[s];
  if (s == SIDE_F) { a.aux[1] = vs.T32; a.aux[2] = nullptr; }     // X.G:  G^T G, T^T G, colSums(G)
  else a.aux[1] = nullptr;                                        // Xt.F: F^T F, colSums(F)
  a.Paux = sd.Paux; a.rows_per_split_aux = sd.rpsaux; a.nsplit_aux = sd.nsaux; a.aux_cnt = sd.cnt;
  a.ctl = h->ctl;
}

// builds the kernel argument blocks (coupling tables included) from the host-side description
static int build_args(resnmtf_handle* h) {
  const int V = h->V;
  double sum_xi = 0.0;
  for (double x : h->xi) sum_xi += x;
  for (int v = 0; v < V; ++v) {
    ViewState& vs = h->views[v];
    if (!vs.has_factors) return h->fail(RESNMTF_ERR_STATE, "set_factors missing for a view");
    if (!vs.owned && !vs.side[SIDE_F].replica && !vs.side[SIDE_G].replica) continue;
    if (int rc = fill_update(h, v, SIDE_F)) return rc;
    if (vs.owned || vs.side[SIDE_G].replica)
      if (int rc = fill_update(h, v, SIDE_G)) return rc;
    if (!vs.owned) continue;       // (replicas only ever run the update kernels)
    if (!vs.has_x) return h->fail(RESNMTF_ERR_STATE, "set_view missing for an owned view");
    // --- streaming passes
    fill_pass(h, v, SIDE_F);
    fill_pass(h, v, SIDE_G);
    // --- k x k side kernels
    KKFArgs& kf = vs.argKF;
    kf = KKFArgs{};
    kf.k = vs.k; kf.S = vs.S; kf.part = vs.side[SIDE_F].part; kf.nblk = vs.side[SIDE_F].nblk;
    kf.FtF = vs.FtF; kf.FtFS = vs.FtFS; kf.Ma_G = vs.side[SIDE_G].Ma; kf.Md_G = vs.side[SIDE_G].Md; kf.cF = vs.cF;
    KKSArgs& ks = vs.argKS;
    ks = KKSArgs{};
    ks.k = vs.k; ks.mode = 1; ks.part = vs.side[SIDE_G].part; ks.nblk = vs.side[SIDE_G].nblk;
    ks.FtF = vs.FtF; ks.FtFS = vs.FtFS; ks.cF = vs.cF;
    ks.S = vs.S; ks.lambda = vs.side[SIDE_F].lm; ks.mu = vs.side[SIDE_G].lm; ks.Ma_F = vs.side[SIDE_F].Ma; ks.Md_F = vs.side[SIDE_F].Md;
    ks.xnorm2 = vs.xnorm2;
    ks.err = h->err; ks.err_stride = V; ks.err_col = v; ks.err_cap = h->err_cap;
    ks.err_host = h->err_host_dev; ks.ctl_host = h->ctl_host_dev;
    ks.sblock = vs.sblk;
    ks.ctl = h->ctl; ks.last_view = (v == h->last_owned) ? 1 : 0; ks.n_views = V; ks.tol = -1.0;
    {
      double sigma = 0.0;
      for (int i = 0; i < V; ++i) sigma += h->xi[(size_t)i + (size_t)v * V];      // sum(xi[, v])  (:231,:233)
      ks.restricted = (sum_xi != 0.0) ? 1 : 0;                                     // whole matrix (:226)
      ks.sigma = sigma;
      ks.n_couple = 0;
      for (int i = 0; i < V && ks.restricted; ++i) {
        const double wgt = h->xi[(size_t)i + (size_t)v * V];
        if (wgt == 0.0 || i == v) continue;                                        // utils.r:42
        if (h->views[i].k != vs.k) return h->fail(RESNMTF_ERR_INVALID, "xi-coupled views need equal k");
        SCouple& c = ks.couple[ks.n_couple++];
        c.S = h->views[i].S;      // running list: updated in place, in view order, on the side stream
        c.weight = wgt;
      }
    }
  }
  build_chain(h, SIDE_F);
  build_chain(h, SIDE_G);
  build_wide_chain(h);
  if (h->sliced)
    if (int rc = build_slice_chain(h)) return rc;
  return RESNMTF_OK;
}

int resnmtf_reserve_sweeps(resnmtf_handle* h, int sweeps) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (sweeps < 1) return h->fail(RESNMTF_ERR_INVALID, "sweeps must be positive");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  return ensure_err_capacity(h, sweeps);
}

// allow_resume: resnmtf_run directly after a completed resnmtf_run with nothing set in between -- the device state
// (X.G slabs, F coefficients, Gram partials) is bit for bit what the run prologue would recompute, so only the loop
// control is reset, in stream order, without a host synchronisation
static int prepare_impl(resnmtf_handle* h, bool allow_resume, bool keep_ctl = false) {
  if (!h->prepared) {
    if (!h->ladder.empty() || !h->exact.empty()) HIP_TRY(h, hipStreamSynchronize(h->stream));   // (a graph may still be executing:
    destroy_graphs(h);                                                                           //  resnmtf_run returns on a counter)
    if (int rc = build_args(h)) return rc;
    h->prepared = true;
  }
  const bool resume = allow_resume && h->resume_ok;
  if (resume && keep_ctl && h->ctl_clean && h->next_base < (1 << 30)) {      // not even a memset
    h->sweep_base = h->next_base;
    return RESNMTF_OK;
  }
  h->sweep_base = h->next_base = 0;
  std::memset(h->ctl_host, 0, sizeof(SweepCtl));
  HIP_TRY(h, hipMemsetAsync(h->ctl, 0, sizeof(SweepCtl), h->stream));      // all-zero bytes = SweepCtl{}
  if (h->view_sweep) HIP_TRY(h, hipMemsetAsync(h->view_sweep, 0, ((size_t)h->V + 1) * sizeof(int), h->stream));
  if (resume) return RESNMTF_OK;
  // run prologue: F coefficients and the first X.G pass of every owned view
  h->resume_ok = false;
  for (const auto& v : h->views)
    if (v.owned && v.fuse_cnt) HIP_TRY(h, hipMemsetAsync(v.fuse_cnt, 0, 4 * sizeof(int), h->stream));
  for (const auto& v : h->views)
    if (v.owned) enqueue_prologue(h, v);
  HIP_TRY(h, hipGetLastError());
  return RESNMTF_OK;
}

int resnmtf_prepare(resnmtf_handle* h) {
  if (!h) return RESNMTF_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  if (h->opt.slice_p2p) {      // the arrival counters only count up: one prepare per handle (the driver prepares once)
    if (!h->p2p_ready) return h->fail(RESNMTF_ERR_STATE, "slice_p2p: import every rank's buffers first (resnmtf_p2p_import)");
    if (h->p2p_prepared) return h->fail(RESNMTF_ERR_STATE, "slice_p2p: a handle is prepared once (its arrival counters are cumulative)");
    h->p2p_prepared = true;
  }
  return prepare_impl(h, false);
}

int resnmtf_phase(resnmtf_handle* h, int v, int phase, int sweep) {
  if (int rc = check_view(h, v)) return rc;
  if (!h->prepared) return h->fail(RESNMTF_ERR_STATE, "resnmtf_prepare has not been called");
  const ViewState& vs = h->views[v];
  if (!vs.owned && !(vs.side[SIDE_F].replica && phase == RESNMTF_PHASE_F) && phase != RESNMTF_PHASE_F_ALL && phase != RESNMTF_PHASE_LOCAL_SWEEP &&
      phase != RESNMTF_PHASE_G_ALL && phase != RESNMTF_PHASE_S_ALL)
    return h->fail(RESNMTF_ERR_STATE, "phase on a view this handle does not own");
  if (phase >= RESNMTF_PHASE_XTF && phase <= RESNMTF_PHASE_S_ALL && !h->opt.replicate_gs)
    return h->fail(RESNMTF_ERR_STATE, "this phase needs a handle created with replicate_gs = 1");
  if (phase >= RESNMTF_PHASE_SLICE_F && phase <= RESNMTF_PHASE_SLICE_XG && !h->sliced)
    return h->fail(RESNMTF_ERR_STATE, "this phase needs a handle created with slice_chains = 1");
  if (h->sliced && phase != RESNMTF_PHASE_S_ALL && !(phase >= RESNMTF_PHASE_SLICE_F && phase <= RESNMTF_PHASE_SLICE_XG))
    return h->fail(RESNMTF_ERR_STATE, "slice_chains: use PHASE_SLICE_F / SLICE_XTF / SLICE_G / SLICE_XG / S_ALL");
  if ((phase == RESNMTF_PHASE_SLICE_XTF || phase == RESNMTF_PHASE_SLICE_XG) && !vs.owned)
    return h->fail(RESNMTF_ERR_STATE, "phase on a view this handle does not own");
  if (h->block_p2p && !h->opt.replicate_gs && phase != RESNMTF_PHASE_LOCAL_SWEEP)
    return h->fail(RESNMTF_ERR_STATE, "slice_p2p with replicate_f alone: the sweep is RESNMTF_PHASE_LOCAL_SWEEP (one exchange per sweep)");
  if (h->opt.replicate_gs && (phase == RESNMTF_PHASE_G || phase == RESNMTF_PHASE_LOCAL_SWEEP))
    return h->fail(RESNMTF_ERR_STATE, "replicate_gs: use PHASE_XTF / G_ALL / XG / S_ALL instead of PHASE_G");
  if (sweep < 0) return h->fail(RESNMTF_ERR_INVALID, "negative sweep index");
  if (sweep >= h->err_cap) return h->fail(RESNMTF_ERR_STATE, "sweep beyond the reserved error buffer (resnmtf_reserve_sweeps)");
  h->resume_ok = false;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (h->opt.time_kernels && h->ev_used + 64 > h->ev.size())
    if (int rc = flush_timing(h)) return rc;
  // convergence mode of the phase API (resnmtf_set_stop_tolerance): the replicated S chain runs the stop test, every kernel
  // of a checked phase leaves at once when the flag is up
  const double tol = h->opt.replicate_gs ? h->phase_tol : -1.0;
  const bool checked = tol >= 0.0;
  switch (phase) {
    case RESNMTF_PHASE_F: enqueue_phase_f(h, vs, false); break;
    case RESNMTF_PHASE_G: enqueue_phase_g(h, vs, -1.0, false); break;
    case RESNMTF_PHASE_S: break;   // S is complete behind PHASE_G on the handle's stream
    case RESNMTF_PHASE_F_ALL: enqueue_phase_f_all(h, checked); break;
    case RESNMTF_PHASE_LOCAL_SWEEP:
      if (h->block_p2p) {
        // peer-store form of the one-exchange layout: the F chain waits for the V blocks stored after sweep t - 1 (the first
        // ones travel by the caller's collective after resnmtf_prepare), says so to every rank once it has read them, and the
        // own block of this sweep is stored only after every rank has said so (the ack has long arrived: two passes lie between)
        if (sweep > 0 || h->opt.slice_p2p == 2) HIP_TRY(h, p2p_wait(h, 0, 0, sweep, 0));
        enqueue_phase_f_all(h);
        p2p_signal(h, 1);
        for (const auto& w : h->views)
          if (w.owned) enqueue_phase_g(h, w, -1.0, false);
        HIP_TRY(h, p2p_wait(h, 1, 1, sweep, 1));
        for (const auto& w : h->views)
          if (w.owned) push_block(h, w, SIDE_F);
        p2p_signal(h, 0);
        break;
      }
      if (int rc = launch_local_sweep(h)) return rc;
      break;
    // block_p2p with the replicated G / S chains: the own T block is stored to the peers behind the Xt.F pass, the own U rows
    // and S block behind the X.G pass; G_ALL / S_ALL wait for the V arrivals of their sweep.  Single arenas: the sweep's own
    // order keeps a writer behind its readers, and what every rank computes itself (coefficients,
    // lambda, mu) is never stored to a peer
    case RESNMTF_PHASE_XTF:
      launch_pass(h, vs, false, 1, tol, checked); launch_fold(h, vs, SIDE_G);
      if (h->block_p2p) { push_block(h, vs, SIDE_G); p2p_signal(h, 1); }
      break;
    case RESNMTF_PHASE_G_ALL:
      if (h->block_p2p) HIP_TRY(h, p2p_wait(h, 1, 2, sweep, 1));
      if (h->wchain_ok[1]) { launch_wide_chain(h, 1, checked); break; }
      if (enqueue_chain(h, SIDE_G, true, checked)) break;      // (the G form always reads one folded slab per view)
      for (const auto& w : h->views)
        if (w.owned || w.side[SIDE_G].replica) launch_update(h, w, 1, checked);
      break;
    case RESNMTF_PHASE_XG:
      launch_pass(h, vs, true, 1, tol, checked); launch_fold(h, vs, SIDE_F);
      if (h->block_p2p) { push_block(h, vs, SIDE_F); p2p_signal(h, 0); }
      break;
    // slice_p2p: every phase first waits (in stream order, hipStreamWaitValue32) until the V arrivals of the exchange that
    // feeds it are in, and ends with one arrival on every rank's counter of the exchange it fed with peer stores.
    // Arrivals so far: U + S blocks V (t + 2) after sweep t's X.G (the run prologue is the first), the others V (t + 1).
    case RESNMTF_PHASE_S_ALL:
      if (h->opt.slice_p2p) HIP_TRY(h, p2p_wait(h, 0, 3, sweep, h->block_p2p ? 1 : 2));
      if (int rc = launch_s_chain(h, checked)) return rc;
      break;
    case RESNMTF_PHASE_SLICE_F:
      if (h->opt.slice_p2p) HIP_TRY(h, p2p_wait(h, 0, 4, sweep, 1));
      launch_wide_chain(h, 0, checked, true);
      if (h->opt.slice_p2p) p2p_signal(h, 1);
      break;
    case RESNMTF_PHASE_SLICE_XTF:
      if (h->opt.slice_p2p) HIP_TRY(h, p2p_wait(h, 1, 5, sweep, 1));
      launch_slice_unpack(h, vs, 0, checked);
      launch_pass(h, vs, false, 1, tol, checked);
      launch_slice_pack(h, vs, false, checked);
      if (h->opt.slice_p2p) p2p_signal(h, 2);
      break;
    case RESNMTF_PHASE_SLICE_G:
      if (h->opt.slice_p2p) HIP_TRY(h, p2p_wait(h, 2, 6, sweep, 1));
      launch_wide_chain(h, 1, checked, true);
      if (h->opt.slice_p2p) p2p_signal(h, 3);
      break;
    case RESNMTF_PHASE_SLICE_XG:
      if (h->opt.slice_p2p) HIP_TRY(h, p2p_wait(h, 3, 7, sweep, 1));
      launch_slice_unpack(h, vs, 1, checked);
      launch_pass(h, vs, true, 1, tol, checked);
      launch_slice_pack(h, vs, true, checked);
      if (h->opt.slice_p2p) p2p_signal(h, 0);
      break;
    default: return h->fail(RESNMTF_ERR_INVALID, "unknown phase");
  }
  HIP_TRY(h, hipGetLastError());
  return RESNMTF_OK;
}

int resnmtf_run(resnmtf_handle* h, int n_iters, double tol, int max_iters, double* all_err, int err_capacity,
                int* iters_done) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (iters_done) *iters_done = 0;
  if (!h->all_owned) return h->fail(RESNMTF_ERR_STATE, "resnmtf_run needs a handle that owns every view; use the phase API");
  if (h->opt.replicate_gs) return h->fail(RESNMTF_ERR_STATE, "resnmtf_run does not drive the replicated G / S chains (replicate_gs); use the phase API");
  if (n_iters < 0) return h->fail(RESNMTF_ERR_INVALID, "n_iters must be >= 0");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  int total;
  double tol_arg;
  if (n_iters > 0) {
    total = n_iters; tol_arg = -1.0;
    if (all_err && err_capacity < n_iters) return h->fail(RESNMTF_ERR_INVALID, "all_err shorter than n_iters");
  } else {
    if (!(tol >= 0.0)) return h->fail(RESNMTF_ERR_INVALID, "tol must be >= 0 in convergence mode");
    tol_arg = tol;
    total = max_iters > 0 ? max_iters : err_capacity;
    if (all_err) total = std::min(total, err_capacity);
    if (total < 1) return h->fail(RESNMTF_ERR_INVALID, "convergence mode needs max_iters > 0 or an all_err buffer");
  }
  // RESNMTF_TRACE_RUN=1: host-side stage times of this call on stderr (diagnostic, tools/time_run_overhead.py)
  static const bool trace = std::getenv("RESNMTF_TRACE_RUN") != nullptr;
  using clk = std::chrono::steady_clock;
  clk::time_point tp[6];
  if (trace) tp[0] = clk::now();
  if (int rc = ensure_err_capacity(h, total)) return rc;
  // (the host mirror of the loop control is rewritten below: the previous run has been waited for)
  if (int rc = prepare_impl(h, true, tol_arg < 0.0)) return rc;
  const int base = h->sweep_base;      // sweeps the device counter stood at when this run began
  h->ctl_clean = false;
  if (trace) tp[1] = clk::now();
  h->resume_ok = false;
  const bool eager = !h->opt.use_graph || h->opt.time_kernels;
  const int batch = std::max(1, h->opt.check_every);
  if (!eager && h->graph_tol != tol_arg) {                 // graphs are captured per stop test
    if (!h->ladder.empty() || !h->exact.empty()) HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the previous run returned on the
    destroy_graphs(h); h->graph_tol = tol_arg;                                                   //  counter: its graph may still execute)
  }
  int enq = 0;
  if (!eager && total > 1) {
    // the first sweep goes out as plain launches: its first kernel starts within a few microseconds, where a graph launch
    // costs the host ~20 us before the GPU sees anything (tools/time_run_overhead.py); the graph launches that follow
    // are enqueued while that sweep runs.  (Same kernels, same arguments: bit for bit the graph's.)
    enqueue_sweep(h, tol_arg);
    enq = 1;
  }
  // fixed-iteration runs shorter than three batches: ONE graph of exactly the sweeps left (captured at the first run of
  // that length, kept for the next ones -- a driver that times `run(20)` after a warm-up call of the same length pays
  // one graph launch, hidden behind the eager first sweep, and no graph-to-graph gaps)
  if (!eager && tol_arg < 0.0 && total - enq > 0 && total - enq < 3 * batch) {
    const int rest = total - enq;
    hipGraphExec_t ex = nullptr;
    for (const auto& g : h->exact)
      if (g.first == rest) ex = g.second;
    if (!ex) {
      if (h->exact.size() >= 4) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));           // (it may be the graph the previous run is still draining)
        (void)hipGraphExecDestroy(h->exact.front().second); h->exact.erase(h->exact.begin());
      }
      if (int rc = capture_graph(h, rest, tol_arg, &ex)) return rc;
      h->exact.emplace_back(rest, ex);
    }
    HIP_TRY(h, hipGraphLaunch(ex, h->stream));
    enq = total;
  }
  if (!eager && enq < total && (h->ladder.empty() || h->ladder.front().first != batch))
    if (int rc = capture_ladder(h, batch, tol_arg)) return rc;
  while (enq < total) {
    const int todo = std::min(batch, total - enq);
    if (eager) {
      for (int s = 0; s < todo; ++s) {
        enqueue_sweep(h, tol_arg);
        if (h->opt.time_kernels && h->ev_used + 8 * (size_t)h->V > h->ev.size())
          if (int rc = flush_timing(h)) return rc;
      }
    } else {
      // a full batch is one launch; a remainder a few (binary ladder), SMALLEST rung first: the host cost of a graph launch
      // grows with its nodes, and everything after the first launch is enqueued while the GPU already works
      int left = todo;
      std::vector<hipGraphExec_t> seq;
      for (const auto& rung : h->ladder)
        while (left >= rung.first) { seq.push_back(rung.second); left -= rung.first; }
      for (auto it = seq.rbegin(); it != seq.rend(); ++it) HIP_TRY(h, hipGraphLaunch(*it, h->stream));
    }
    enq += todo;
    if (tol_arg >= 0.0) {     // convergence mode (R/main.r:50-81): look at the (mirrored) device flag between batches
      HIP_TRY(h, hipGetLastError());
      if (int rc = sync_both(h)) return rc;
      if (h->ctl_host->done) break;
    }
  }
  HIP_TRY(h, hipGetLastError());
  if (trace) tp[2] = clk::now();
  if (tol_arg < 0.0 && !h->opt.time_kernels && h->last_owned >= 0 && h->opt.wait_mode == 0) {
    // fixed-iteration runs: wait for the sweep counter the LAST k x k job mirrors into pinned host memory (errors are
    // written, and fenced, before it) instead of a stream synchronisation, whose wake-up costs ~10 us of a 0.9 ms run;
    // the stream may still be draining the last launch's workgroups -- every other entry point synchronises it first.
    // Bounded: after 20 ms without progress the stream synchronisation below takes over.
    const int want = base + total;
    volatile int* counter = &h->ctl_host->sweep;
    int seen = *counter;
    auto t_last = clk::now();
    while (seen != want) {
      const int now = *counter;
      if (now != seen) { seen = now; t_last = clk::now(); }
      else if (std::chrono::duration<double, std::milli>(clk::now() - t_last).count() > 20.0) break;
      for (int p = 0; p < 16; ++p) __builtin_ia32_pause();     // (back off: the core's sibling thread and the memory bus get air)
    }
    if (seen != want)
      if (int rc = sync_both(h)) return rc;
  } else if (int rc = sync_both(h)) return rc;
  if (trace) tp[3] = clk::now();
  if (h->fuse_err && *h->fuse_err) {
    *h->fuse_err = 0;
    h->resume_ok = false;
    return h->fail(RESNMTF_ERR_HIP, "a fused pass launch gave up waiting for its update blocks (pass_fused_kernel): results are invalid");
  }
  const int done_total = h->ctl_host->sweep - base;
  if (tol_arg < 0.0 && done_total != total) return h->fail(RESNMTF_ERR_HIP, "sweep counter mismatch");
  if (all_err && done_total > 0) {
    for (int t = 0; t < done_total; ++t) {        // mean over views (R/main.r:77-78,104-107)
      double sum = 0.0;
      const size_t row = (size_t)((base + t) % h->err_cap) * h->V;
      for (int v = 0; v < h->V; ++v) sum += h->err_host[row + v];
      all_err[t] = sum / (double)h->V;
    }
  }
  if (h->opt.time_kernels)
    if (int rc = flush_timing(h)) return rc;
  if (iters_done) *iters_done = done_total;
  h->resume_ok = true;
  h->ctl_clean = tol_arg < 0.0;        // (a convergence run leaves its stop flag and prev_mean behind)
  h->next_base = base + done_total;
  if (trace) {
    tp[4] = clk::now();
    auto us = [&](int a, int b) { return std::chrono::duration<double, std::micro>(tp[b] - tp[a]).count(); };
    std::fprintf(stderr, "[resnmtf_run] sweeps %d: prepare %.1f us, enqueue %.1f us, wait %.1f us, read-out %.1f us\n", total,
                 us(0, 1), us(1, 2), us(2, 3), us(3, 4));
  }
  return RESNMTF_OK;
}

int resnmtf_get_factors(resnmtf_handle* h, int v, double* F, double* S, double* G, double* lambda, double* mu) {
  if (int rc = check_view(h, v)) return rc;
  ViewState& vs = h->views[v];
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  std::vector<double> tmp;
  if (F) { tmp.resize((size_t)vs.n * vs.k); HIP_TRY(h, hipMemcpy(tmp.data(), vs.side[SIDE_F].W, tmp.size() * sizeof(double), hipMemcpyDeviceToHost)); to_col_major(tmp, vs.n, vs.k, F); }
  if (S) { tmp.resize((size_t)vs.k * vs.k); HIP_TRY(h, hipMemcpy(tmp.data(), vs.S, tmp.size() * sizeof(double), hipMemcpyDeviceToHost)); to_col_major(tmp, vs.k, vs.k, S); }
  if (G) { tmp.resize((size_t)vs.m * vs.k); HIP_TRY(h, hipMemcpy(tmp.data(), vs.side[SIDE_G].W, tmp.size() * sizeof(double), hipMemcpyDeviceToHost)); to_col_major(tmp, vs.m, vs.k, G); }
  if (lambda || mu) {
    if (!vs.owned) return h->fail(RESNMTF_ERR_STATE, "lambda/mu only exist on the owning handle");
    if (lambda) HIP_TRY(h, hipMemcpy(lambda, vs.side[SIDE_F].lm, (size_t)vs.k * sizeof(double), hipMemcpyDeviceToHost));
    if (mu) HIP_TRY(h, hipMemcpy(mu, vs.side[SIDE_G].lm, (size_t)vs.k * sizeof(double), hipMemcpyDeviceToHost));
  }
  return RESNMTF_OK;
}

// The raw state into caller-owned device buffers: the transposes write them in place, ordered with
// `stream` as resnmtf_finalise_device orders its copies; no transient memory.
int resnmtf_get_factors_device(resnmtf_handle* h, int v, double* F, double* S, double* G, double* lambda, double* mu, void* stream) {
  if (int rc = check_view(h, v)) return rc;
  ViewState& vs = h->views[v];
  for (const double* p : {F, S, G, lambda, mu})
    if (p && !on_handle_device(h, p)) return h->fail(RESNMTF_ERR_INVALID, "an output is not device memory of the handle's device (host buffers: resnmtf_get_factors)");
  if ((lambda || mu) && !vs.owned) return h->fail(RESNMTF_ERR_STATE, "lambda/mu only exist on the owning handle");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  HIP_TRY(h, wait_for_caller(h, stream));
  // row-major W [len][k] -> column-major out: W read as the k x len matrix of row stride 1 it also is
  auto emit = [&](const double* W, int len, int k, double* out) {
    hipLaunchKernelGGL(device_factor_transpose_kernel<RESNMTF_DTYPE_F64>, dim3(ceil_div(k, 32) * ceil_div(len, 32)), dim3(256), 0, h->stream,
                       W, 1LL, (long long)k, k, len, out, (long long)len, 1LL);
  };
  if (F) emit(vs.side[SIDE_F].W, vs.n, vs.k, F);
  if (S) emit(vs.S, vs.k, vs.k, S);
  if (G) emit(vs.side[SIDE_G].W, vs.m, vs.k, G);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && lambda) e = hipMemcpyAsync(lambda, vs.side[SIDE_F].lm, (size_t)vs.k * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess && mu) e = hipMemcpyAsync(mu, vs.side[SIDE_G].lm, (size_t)vs.k * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
  // (the handle's stream is drained before the call returns: whatever the caller enqueues afterwards comes after the writes)
  const hipError_t es = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return h->fail_hip("get_factors_device", e);
  return RESNMTF_OK;
}

namespace {
// resnmtf_finalise (outputs on the host) and resnmtf_finalise_device (outputs in device memory, ordered with `stream`)
int finalise_impl(resnmtf_handle* h, int v, double* F, double* S, double* G, double* row_clusters, double* col_clusters,
                  bool to_device, void* stream) {
  if (int rc = check_view(h, v)) return rc;
  ViewState& vs = h->views[v];
  if (to_device)
    for (const double* p : {F, S, G, row_clusters, col_clusters})
      if (p && !on_handle_device(h, p)) return h->fail(RESNMTF_ERR_INVALID, "an output is not device memory of the handle's device (host buffers: resnmtf_finalise)");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  if (to_device) HIP_TRY(h, wait_for_caller(h, stream));
  const hipMemcpyKind kind = to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t nk = (size_t)vs.n * vs.k, mk = (size_t)vs.m * vs.k, kk = (size_t)vs.k * vs.k;
  const size_t total = 2 * (size_t)vs.k + kk + 2 * nk + 2 * mk;
  Scratch sc;
  double* buf = sc.take<double>(total);   // [cF k][cG k][S kk][Fout nk][rc nk][Gout mk][cc mk]
  int* rel = sc.take<int>((size_t)vs.k);
  hipError_t e = sc.error();
  if (e != hipSuccess) return h->fail_hip("hipMalloc", e);
  double *cF = buf, *cG = cF + vs.k, *So = cG + vs.k, *Fo = So + kk, *rc_ = Fo + nk, *Go = rc_ + nk, *cc = Go + mk;
  hipLaunchKernelGGL(colsum_kernel, dim3(vs.k), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n, vs.k, cF);
  hipLaunchKernelGGL(colsum_kernel, dim3(vs.k), dim3(256), 0, h->stream, vs.side[SIDE_G].W, vs.m, vs.k, cG);
  hipLaunchKernelGGL(finalise_s_kernel, dim3(1), dim3(64), 0, h->stream, vs.S, vs.k, cF, cG, So, rel);
  hipLaunchKernelGGL(finalise_factor_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n,
                     vs.k, cF, rel, Fo, rc_);
  hipLaunchKernelGGL(finalise_factor_kernel, dim3((unsigned)((mk + 255) / 256)), dim3(256), 0, h->stream, vs.side[SIDE_G].W, vs.m,
                     vs.k, cG, (const int*)nullptr, Go, cc);
  e = hipGetLastError();
  if (e == hipSuccess && !to_device) e = hipStreamSynchronize(h->stream);
  // (to the device: the copies follow the kernels on the handle's stream, which is drained before the call returns --
  // whatever the caller enqueues afterwards, on any stream, comes after them)
  auto copy = [&](double* dst, const double* src, size_t count) {
    return to_device ? hipMemcpyAsync(dst, src, count * sizeof(double), kind, h->stream) : hipMemcpy(dst, src, count * sizeof(double), kind);
  };
  if (e == hipSuccess && S) e = copy(S, So, kk);
  if (e == hipSuccess && F) e = copy(F, Fo, nk);
  if (e == hipSuccess && G) e = copy(G, Go, mk);
  if (e == hipSuccess && row_clusters) e = copy(row_clusters, rc_, nk);
  if (e == hipSuccess && col_clusters) e = copy(col_clusters, cc, mk);
  if (to_device) { const hipError_t es = hipStreamSynchronize(h->stream); if (e == hipSuccess) e = es; }
  if (e != hipSuccess) return h->fail_hip("finalise", e);
  return RESNMTF_OK;
}
}  // namespace

int resnmtf_finalise(resnmtf_handle* h, int v, double* F, double* S, double* G, double* row_clusters,
                     double* col_clusters) {
  return finalise_impl(h, v, F, S, G, row_clusters, col_clusters, false, nullptr);
}
int resnmtf_finalise_device(resnmtf_handle* h, int v, double* F, double* S, double* G, double* row_clusters,
                            double* col_clusters, void* stream) {
  return finalise_impl(h, v, F, S, G, row_clusters, col_clusters, true, stream);
}

// ---- stability selection (R/stability_analysis.r:302-338): relevance of a sub-sample's biclusters, on the device
int resnmtf_set_reference_clusters(resnmtf_handle* h, int v, int k, const double* row_clusters, const double* col_clusters) {
  if (int rc = check_view(h, v)) return rc;
  if (!row_clusters || !col_clusters) return h->fail(RESNMTF_ERR_INVALID, "row_clusters / col_clusters are NULL");
  if (k < 1 || k > RESNMTF_MAX_K) return h->fail(RESNMTF_ERR_INVALID, "k must be in [1, 64]");
  ViewState& vs = h->views[v];
  const size_t nk = (size_t)vs.n * k, mk = (size_t)vs.m * k;
  std::vector<unsigned char> bytes(nk + mk);       // column-major 0 / 1 doubles -> row-major bytes
  for (int j = 0; j < k; ++j) {
    for (int r = 0; r < vs.n; ++r) {
      const double x = row_clusters[(size_t)j * vs.n + r];
      if (x != 0.0 && x != 1.0) return h->fail(RESNMTF_ERR_INVALID, "row_clusters entries must be 0 or 1");
      bytes[(size_t)r * k + j] = x != 0.0;
    }
    for (int c = 0; c < vs.m; ++c) {
      const double x = col_clusters[(size_t)j * vs.m + c];
      if (x != 0.0 && x != 1.0) return h->fail(RESNMTF_ERR_INVALID, "col_clusters entries must be 0 or 1");
      bytes[nk + (size_t)c * k + j] = x != 0.0;
    }
  }
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  if (vs.ref_cl) { (void)hipFree(vs.ref_cl); vs.ref_cl = nullptr; vs.ref_k = 0; }
  HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&vs.ref_cl), bytes.size()));
  const hipError_t e = hipMemcpy(vs.ref_cl, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(vs.ref_cl); vs.ref_cl = nullptr; return h->fail_hip("set_reference_clusters", e); }
  vs.ref_k = k;
  return RESNMTF_OK;
}

// The same from 0 / 1 matrices that are ALREADY in device memory (resnmtf_view_readback.hip.inc):
// checked and packed on the device into a fresh block, which replaces the view's block only when every entry passed.
// Transient device memory: the two flag words.
int resnmtf_set_reference_clusters_device(resnmtf_handle* h, int v, int k, const resnmtf_device_matrix* row_clusters,
                                          const resnmtf_device_matrix* col_clusters, void* stream) {
  if (int rc = check_view(h, v)) return rc;
  if (!row_clusters || !col_clusters || !row_clusters->ptr || !col_clusters->ptr) return h->fail(RESNMTF_ERR_INVALID, "row_clusters / col_clusters are NULL");
  if (k < 1 || k > RESNMTF_MAX_K) return h->fail(RESNMTF_ERR_INVALID, "k must be in [1, 64]");
  for (const resnmtf_device_matrix* a : {row_clusters, col_clusters}) {
    if (a->dtype != RESNMTF_DTYPE_F64 && a->dtype != RESNMTF_DTYPE_F32 && a->dtype != RESNMTF_DTYPE_F16 && a->dtype != RESNMTF_DTYPE_BF16)
      return h->fail(RESNMTF_ERR_INVALID, "unknown dtype: one of RESNMTF_DTYPE_F64 / _F32 / _F16 / _BF16");
    if (a->row_stride < 0 || a->col_stride < 0) return h->fail(RESNMTF_ERR_INVALID, "negative strides are not supported");
  }
  for (const resnmtf_device_matrix* a : {row_clusters, col_clusters})
    if (!on_handle_device(h, a->ptr))
      return h->fail(RESNMTF_ERR_INVALID, "a cluster matrix is not device memory of the handle's device (host matrices: resnmtf_set_reference_clusters)");
  ViewState& vs = h->views[v];
  const size_t nk = (size_t)vs.n * k, mk = (size_t)vs.m * k;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  unsigned char* fresh = nullptr;
  int bad_host[2] = {0, 0};
  hipError_t e = hipSuccess;
  {
    Scratch sc;
    int* bad = sc.take<int>(2);                        // [0]: a bad entry in row_clusters, [1]: in col_clusters
    if (sc.error() != hipSuccess) return h->fail_hip("hipMalloc set_reference_clusters_device flags", sc.error());
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&fresh), nk + mk));
    e = wait_for_caller(h, stream);
    if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 2 * sizeof(int), h->stream);
    if (e == hipSuccess) {
      // a column-major source (row stride the smaller) is read with threads along the rows, through the LDS tile
      auto pack = [&](const resnmtf_device_matrix* a, int len, unsigned char* dst, int* flag) {
        const dim3 grid((unsigned)ceil_div(len, 32) * (unsigned)ceil_div(k, 32));
        pick_int<RESNMTF_DTYPE_F64, RESNMTF_DTYPE_F32, RESNMTF_DTYPE_F16, RESNMTF_DTYPE_BF16>(a->dtype, [&](auto dt) {
          pick_bools([&](auto along_r) {
            hipLaunchKernelGGL((reference_clusters_pack_kernel<decltype(dt)::value, decltype(along_r)::value>), grid, dim3(256), 0, h->stream,
                               a->ptr, a->row_stride, a->col_stride, len, k, dst, flag);
          }, a->row_stride < a->col_stride);
        });
      };
      pack(row_clusters, vs.n, fresh, bad);
      pack(col_clusters, vs.m, fresh + nk, bad + 1);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad_host, bad, sizeof(bad_host), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);   // the sources may be freed on return
    if (e == hipSuccess) e = es;
  }
  if (e != hipSuccess) { (void)hipFree(fresh); return h->fail_hip("set_reference_clusters_device", e); }
  if (bad_host[0] || bad_host[1]) {
    (void)hipFree(fresh);
    return h->fail(RESNMTF_ERR_INVALID, bad_host[0] ? "row_clusters entries must be 0 or 1" : "col_clusters entries must be 0 or 1");
  }
  if (vs.ref_cl) (void)hipFree(vs.ref_cl);
  vs.ref_cl = fresh;
  vs.ref_k = k;
  return RESNMTF_OK;
}

namespace {
// resnmtf_relevance (flags == nullptr) and resnmtf_relevance_masked (k flag bytes, indexed by F column)
int relevance_impl(resnmtf_handle* h, int v, resnmtf_handle* ref, int v_ref, const int* rows, const int* cols,
                   const unsigned char* flags, double* relevance) {
  if (h->opt.device_id != ref->opt.device_id) return h->fail(RESNMTF_ERR_INVALID, "handles live on different devices");
  const ViewState& vs = h->views[v];
  const ViewState& rs = ref->views[v_ref];
  if (!rs.ref_cl) return h->fail(RESNMTF_ERR_STATE, "no reference clusters set on the reference view");
  if (!vs.has_factors) return h->fail(RESNMTF_ERR_STATE, "the view has no factors");
  if (rs.ref_k != vs.k) return h->fail(RESNMTF_ERR_INVALID, "the reference clusters' k differs from the view's k");
  for (int r = 0; r < vs.n; ++r) if (rows[r] < 0 || rows[r] >= rs.n) return h->fail(RESNMTF_ERR_INVALID, "row index out of range");
  for (int c = 0; c < vs.m; ++c) if (cols[c] < 0 || cols[c] >= rs.m) return h->fail(RESNMTF_ERR_INVALID, "column index out of range");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  const int k = vs.k;
  const size_t kk = (size_t)k * k, side = kk + 2 * (size_t)k;
  // [cF k][cG k][S_out kk][out k] doubles | [relations k][rows n][cols m] ints | [counts 2 side] unsigned
  // (masked: then [flags k] bytes)
  const size_t n_dbl = 3 * (size_t)k + kk, n_int = (size_t)k + vs.n + vs.m;
  const size_t n_bytes = n_dbl * sizeof(double) + n_int * sizeof(int) + 2 * side * sizeof(unsigned int);
  Scratch sc;
  char* buf = sc.take<char>(n_bytes + (flags ? (size_t)k : 0));
  if (!buf) return h->fail_hip("relevance hipMalloc", sc.error());
  double *cF = reinterpret_cast<double*>(buf), *cG = cF + k, *So = cG + k, *out = So + kk;
  int *rel = reinterpret_cast<int*>(buf + n_dbl * sizeof(double)), *idx = rel + k;
  unsigned int* counts = reinterpret_cast<unsigned int*>(idx + vs.n + vs.m);
  unsigned char* dflags = flags ? reinterpret_cast<unsigned char*>(buf + n_bytes) : nullptr;
  hipError_t e = hipMemcpyAsync(idx, rows, (size_t)vs.n * sizeof(int), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(idx + vs.n, cols, (size_t)vs.m * sizeof(int), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess && flags) e = hipMemcpyAsync(dflags, flags, (size_t)k, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 2 * side * sizeof(unsigned int), h->stream);
  if (e == hipSuccess) {
    // the clusters resnmtf_finalise would emit: same kernels, same reductions, same first-max relations
    hipLaunchKernelGGL(colsum_kernel, dim3(k), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n, k, cF);
    hipLaunchKernelGGL(colsum_kernel, dim3(k), dim3(256), 0, h->stream, vs.side[SIDE_G].W, vs.m, k, cG);
    hipLaunchKernelGGL(finalise_s_kernel, dim3(1), dim3(64), 0, h->stream, vs.S, k, cF, cG, So, rel);
    const int grid_r = std::max(1, std::min(128, ceil_div(ceil_div(vs.n, 64), 4)));
    const int grid_c = std::max(1, std::min(128, ceil_div(ceil_div(vs.m, 64), 4)));
    if (!flags) {
      hipLaunchKernelGGL(relevance_count_kernel<false>, dim3(grid_r), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n, k, cF, (const int*)rel,
                         (const unsigned char*)rs.ref_cl, (const int*)idx, counts, (const int*)nullptr, (const unsigned char*)nullptr);
      hipLaunchKernelGGL(relevance_count_kernel<false>, dim3(grid_c), dim3(256), 0, h->stream, vs.side[SIDE_G].W, vs.m, k, cG, (const int*)nullptr,
                         (const unsigned char*)(rs.ref_cl + (size_t)rs.n * k), (const int*)(idx + vs.n), counts + side,
                         (const int*)nullptr, (const unsigned char*)nullptr);
    } else {                // the removal's zeroed cluster columns: flags through the relations, on both sides
      hipLaunchKernelGGL(relevance_count_kernel<true>, dim3(grid_r), dim3(256), 0, h->stream, vs.side[SIDE_F].W, vs.n, k, cF, (const int*)rel,
                         (const unsigned char*)rs.ref_cl, (const int*)idx, counts, (const int*)rel, (const unsigned char*)dflags);
      hipLaunchKernelGGL(relevance_count_kernel<true>, dim3(grid_c), dim3(256), 0, h->stream, vs.side[SIDE_G].W, vs.m, k, cG, (const int*)nullptr,
                         (const unsigned char*)(rs.ref_cl + (size_t)rs.n * k), (const int*)(idx + vs.n), counts + side,
                         (const int*)rel, (const unsigned char*)dflags);
    }
    hipLaunchKernelGGL(relevance_epilogue_kernel, dim3(1), dim3(64), 0, h->stream, k, (const unsigned int*)counts,
                       (const unsigned int*)(counts + side), out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(relevance, out, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return h->fail_hip("relevance", e);
  return RESNMTF_OK;
}
}  // namespace

int resnmtf_relevance(resnmtf_handle* h, int v, resnmtf_handle* ref, int v_ref, const int* rows, const int* cols,
                      double* relevance) {
  if (int rc = check_view(h, v)) return rc;
  if (!ref || v_ref < 0 || v_ref >= ref->V) return h->fail(RESNMTF_ERR_INVALID, "bad reference handle / view");
  if (!rows || !cols || !relevance) return h->fail(RESNMTF_ERR_INVALID, "rows / cols / relevance are NULL");
  return relevance_impl(h, v, ref, v_ref, rows, cols, nullptr, relevance);
}

int resnmtf_relevance_masked(resnmtf_handle* h, int v, resnmtf_handle* ref, int v_ref, const int* rows, const int* cols,
                             const unsigned char* flags, double* relevance) {
  if (int rc = check_view(h, v)) return rc;
  if (!ref || v_ref < 0 || v_ref >= ref->V) return h->fail(RESNMTF_ERR_INVALID, "bad reference handle / view");
  if (!rows || !cols || !flags || !relevance) return h->fail(RESNMTF_ERR_INVALID, "rows / cols / flags / relevance are NULL");
  return relevance_impl(h, v, ref, v_ref, rows, cols, flags, relevance);
}

// ---- bisilhouette (R/obtain_bicl.r:189-199): per-member silhouettes of a view's biclusters (resnmtf_bisil.hip.inc)
namespace {
// What resnmtf_bisil / _sparse and resnmtf_bisil_device share: the sizing of a call from its counts (bisil_plan), the
// checked workspace (bisil_take_workspace) and the launches of every side and bicluster (bisil_enqueue_sides).
struct BisilPlan {
  size_t g_floats = 1, part_dbl = 1, upad_max = 64;
  int chunks[2][RESNMTF_MAX_K] = {}, chunk_tiles[2][RESNMTF_MAX_K] = {};
  int kq = 1;                             // the per-thread bicluster sums of bisil_dist_kernel
  size_t g_dbl() const { return (g_floats + 1) / 2; }
  size_t work_dbl() const { return g_dbl() + upad_max + part_dbl; }      // [G g_floats f32 (rounded to doubles)][norm2][partial]
};
// n_u: |U| per side; cnt[sd][j] = the members of bicluster j on side sd (= |mpos_j| for an active j).
// sizes: G <= max over sides and biclusters of |features| x U_pad floats (<= one padded X image, which a sparse view
// never held: checked against the device's free memory, bisil_take_workspace); partials of one bicluster
void bisil_plan(int k, unsigned long long active, const int n_u[2], const int* const cnt[2], BisilPlan& p) {
  p = BisilPlan();
  for (int sd = 0; sd < 2; ++sd) {
    const int upad = round_up(n_u[sd], BISIL_TILE);
    p.upad_max = std::max<size_t>(p.upad_max, upad);
    for (int j = 0; j < k; ++j) {
      if (!((active >> j) & 1ull)) continue;
      const int n_mem = cnt[sd][j];
      // enough workgroups to fill the device: the others are split into chunks of whole tiles, summed in order later
      // (the rule and the kq table: resnmtf_bisil_plan.h, one statement for this unit and resnmtf_fp64_bisil)
      const BisilChunks c = bisil_chunk_rule(n_u[sd], n_mem);
      p.chunk_tiles[sd][j] = c.chunk_tiles;
      p.chunks[sd][j] = c.chunks;
      p.g_floats = std::max(p.g_floats, (size_t)cnt[1 - sd][j] * upad);
      p.part_dbl = std::max(p.part_dbl, (size_t)p.chunks[sd][j] * n_mem * k);
    }
  }
  p.kq = bisil_kq(k);
}

// `bytes` of transient device memory from `sc`, refused with the sizes when the device has not that much free
int bisil_take_workspace(resnmtf_handle* h, Scratch& sc, size_t bytes, size_t g_floats, char** buf) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    return h->fail(RESNMTF_ERR_ALLOC, "bisil workspace: " + std::to_string(bytes) + " bytes asked for (" + std::to_string(g_floats * sizeof(float)) +
                   " of them the restricted block, features x padded members), " + std::to_string(free_b) + " free on the device");
  *buf = sc.take<char>(bytes);
  if (const hipError_t ea = sc.error(); ea != hipSuccess) {
    (void)hipGetLastError();
    return h->fail(ea == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP,
                   "bisil workspace: hipMalloc of " + std::to_string(bytes) + " bytes asked for: " + hipGetErrorString(ea));
  }
  return RESNMTF_OK;
}

struct BisilLists {                       // one call's metadata in device memory, per side (and active bicluster)
  const unsigned long long* umask[2] = {};
  const int* upts[2] = {};
  const int* cnt[2] = {};
  const int* rank[2] = {};                // sparse views only
  const int* mpos[2][RESNMTF_MAX_K] = {};
  const int* feat[2][RESNMTF_MAX_K] = {};
};

// the launches of every side and active bicluster on the handle's stream; work: BisilPlan::work_dbl() doubles; sil:
// [n k][m k], zeroed by the caller
hipError_t bisil_enqueue_sides(resnmtf_handle* h, const ViewState& vs, int k, int metric, bool from_sparse, unsigned long long active,
                               const int n_u_side[2], const int* const cnt[2], const BisilPlan& plan, const BisilLists& d,
                               char* work, double* sil) {
  float* G = reinterpret_cast<float*>(work);
  double* norm2 = reinterpret_cast<double*>(work) + plan.g_dbl();
  double* partial = norm2 + plan.upad_max;
  hipError_t e = hipMemsetAsync(norm2, 0, plan.upad_max * sizeof(double), h->stream);
  for (int sd = 0; sd < 2 && e == hipSuccess; ++sd) {
    const int n_u = n_u_side[sd], upad = round_up(n_u, BISIL_TILE);
    const int n_pts = sd == 0 ? vs.n : vs.m;
    const float* img = vs.side[sd].X;             // rows: X(row, col) = X^T image (col, row); columns: X image (row, col)
    const size_t ld = vs.side[sd].ldx;
    double* out = sil + (sd == 0 ? 0 : (size_t)vs.n * k);
    for (int j = 0; j < k && e == hipSuccess; ++j) {
      if (!((active >> j) & 1ull)) continue;
      const int nf = cnt[1 - sd][j], n_mem = cnt[sd][j];
      const int* feat = d.feat[sd][j];
      const int* mpos = d.mpos[sd][j];
      const size_t total = (size_t)nf * upad;
      if (!from_sparse) {
        hipLaunchKernelGGL(bisil_gather_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0,
                           h->stream, (const float*)img, ld, feat, nf, d.upts[sd], n_u, upad, G);
      } else {      // rows: the features are columns, their entries in the CSC; columns: rows, in the CSR
        if ((e = hipMemsetAsync(G, 0, total * sizeof(float), h->stream)) != hipSuccess) break;
        hipLaunchKernelGGL(bisil_scatter_kernel, dim3((unsigned)std::min(ceil_div(nf, BISIL_THREADS / 64), 65536)), dim3(BISIL_THREADS), 0,
                           h->stream, (const long long*)vs.side[1 - sd].sp_ptr, (const int*)vs.side[1 - sd].sp_idx,
                           (const float*)vs.side[1 - sd].sp_val, feat, nf, d.rank[sd], upad, G);
      }
      if (metric == BISIL_COSINE)
        hipLaunchKernelGGL(bisil_norm_kernel, dim3(ceil_div(upad, 256)), dim3(256), 0, h->stream, (const float*)G, nf, upad, norm2);
      const dim3 grid(ceil_div(n_mem, BISIL_TILE), plan.chunks[sd][j]);
      bisil_launch_dist(metric, plan.kq, grid, h->stream, G, nf, upad, n_u, mpos, n_mem, d.umask[sd], norm2, k, plan.chunk_tiles[sd][j], partial);
      hipLaunchKernelGGL(bisil_epilogue_kernel, dim3(ceil_div(n_mem, 4)), dim3(256), 0, h->stream, (const double*)partial,
                         plan.chunks[sd][j], n_mem, k, j, mpos, d.umask[sd], d.upts[sd], d.cnt[sd], active, n_pts, out);
      e = hipGetLastError();
    }
  }
  return e;
}

// the refusals of a view's state, shared by the three entries; *from_sparse: asked for (resnmtf_bisil / _sparse) or, with
// `dispatch`, taken from the view's storage (resnmtf_bisil_device)
int bisil_check_state(resnmtf_handle* h, const ViewState& vs, bool dispatch, bool* from_sparse) {
  if (dispatch) *from_sparse = vs.sparse;
  if (*from_sparse && !vs.sparse) return h->fail(RESNMTF_ERR_STATE, "bisil_sparse of a dense view: use resnmtf_bisil");
  if (!*from_sparse && vs.sparse) return h->fail(RESNMTF_ERR_STATE, "bisil of a sparse view is not supported (no dense fp32 image)");
  if (!vs.owned || !vs.has_x) return h->fail(RESNMTF_ERR_STATE, "no data on this handle for the view");
  if (!*from_sparse && (!vs.side[SIDE_G].X || !vs.side[SIDE_F].X))
    return h->fail(RESNMTF_ERR_STATE, "bisil needs the view's fp32 images (the view holds only a 2-byte image)");
  return RESNMTF_OK;
}

// resnmtf_bisil (from_sparse = false: G gathered from the fp32 images) and resnmtf_bisil_sparse (true: G scattered from
// the CSC / CSR copies); everything but the view's storage check and the build of G is common
int bisil_impl(resnmtf_handle* h, int v, int k, const double* row_clusters, const double* col_clusters, int metric,
               double* row_sil, double* col_sil, bool from_sparse) {
  if (int rc = check_view(h, v)) return rc;
  if (!row_clusters || !col_clusters || !row_sil || !col_sil)
    return h->fail(RESNMTF_ERR_INVALID, "row_clusters / col_clusters / row_sil / col_sil are NULL");
  if (k < 1 || k > RESNMTF_MAX_K) return h->fail(RESNMTF_ERR_INVALID, "k must be in [1, 64]");
  if (metric < BISIL_EUCLIDEAN || metric > BISIL_COSINE)
    return h->fail(RESNMTF_ERR_INVALID, "metric must be 0 (euclidean), 1 (manhattan) or 2 (cosine)");
  const ViewState& vs = h->views[v];
  if (int rc = bisil_check_state(h, vs, false, &from_sparse)) return rc;
  const int n = vs.n, m = vs.m;
  // the membership words, counts, U, masks and member lists of both sides (resnmtf_bisil_plan.h: shared with
  // resnmtf_fp64_bisil); per side the features of bicluster j are the other side's members of j, as point indices
  BisilHostLists lists;
  if (const int which = bisil_build_lists(n, m, k, row_clusters, col_clusters, lists))
    return h->fail(RESNMTF_ERR_INVALID, which == 1 ? "row_clusters entries must be 0 or 1" : "col_clusters entries must be 0 or 1");
  const unsigned long long active = lists.active;              // biclusters with rows and columns
  const BisilHostSide (&side)[2] = lists.side;
  auto features = [&](int sd, int j) { return lists.features(sd, j); };
  std::fill(row_sil, row_sil + (size_t)n * k, 0.0);
  std::fill(col_sil, col_sil + (size_t)m * k, 0.0);
  if (!active) return RESNMTF_OK;
  const int n_u[2] = {(int)side[0].upts.size(), (int)side[1].upts.size()};
  const int* const cnt[2] = {side[0].cnt.data(), side[1].cnt.data()};
  BisilPlan plan;
  bisil_plan(k, active, n_u, cnt, plan);
  // host image of the metadata: per side [umask (u64) | upts | cnt | (sparse: rank) | per active j: mpos_j | feat_j];
  // rank[p] = the position of point p in U or -1 (bisil_scatter_kernel)
  std::vector<unsigned long long> meta;
  size_t off_mask[2], off_pts[2], off_cnt[2], off_rank[2] = {0, 0}, off_mpos[2][RESNMTF_MAX_K], off_feat[2][RESNMTF_MAX_K];
  {
    std::vector<int> ints;
    auto put = [&](const std::vector<int>& a) { const size_t o = ints.size(); ints.insert(ints.end(), a.begin(), a.end()); return o; };
    for (int sd = 0; sd < 2; ++sd) {
      const BisilHostSide& s = side[sd];
      off_pts[sd] = put(s.upts);
      off_cnt[sd] = put(s.cnt);
      if (from_sparse) {
        std::vector<int> rank(s.n_pts, -1);
        for (size_t u = 0; u < s.upts.size(); ++u) rank[s.upts[u]] = (int)u;
        off_rank[sd] = put(rank);
      }
      for (int j = 0; j < k; ++j) {
        if (!((active >> j) & 1ull)) continue;
        off_mpos[sd][j] = put(s.mpos[j]);
        off_feat[sd][j] = put(features(sd, j));
      }
    }
    ints.resize(round_up((int)ints.size(), 2), 0);
    const size_t n_mask = side[0].umask.size() + side[1].umask.size();
    meta.resize(n_mask + ints.size() / 2);
    off_mask[0] = 0; off_mask[1] = side[0].umask.size();
    std::copy(side[0].umask.begin(), side[0].umask.end(), meta.begin());
    std::copy(side[1].umask.begin(), side[1].umask.end(), meta.begin() + off_mask[1]);
    std::memcpy(meta.data() + n_mask, ints.data(), ints.size() * sizeof(int));
    for (int sd = 0; sd < 2; ++sd) {      // int offsets -> offsets from the buffer's start, in ints
      off_pts[sd] += 2 * n_mask; off_cnt[sd] += 2 * n_mask; off_rank[sd] += 2 * n_mask;
      for (int j = 0; j < k; ++j) { off_mpos[sd][j] += 2 * n_mask; off_feat[sd][j] += 2 * n_mask; }
    }
  }
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  // [G | norm2 | partial (BisilPlan::work_dbl)][sil n k + m k] doubles | meta
  const size_t sil_dbl = (size_t)n * k + (size_t)m * k;
  const size_t bytes = (plan.work_dbl() + sil_dbl) * sizeof(double) + meta.size() * sizeof(unsigned long long);
  Scratch sc;
  char* buf = nullptr;
  if (int rc = bisil_take_workspace(h, sc, bytes, plan.g_floats, &buf)) return rc;
  double* sil = reinterpret_cast<double*>(buf) + plan.work_dbl();
  unsigned long long* dmeta = reinterpret_cast<unsigned long long*>(sil + sil_dbl);
  const int* dints = reinterpret_cast<const int*>(dmeta);
  BisilLists d;
  for (int sd = 0; sd < 2; ++sd) {
    d.umask[sd] = dmeta + off_mask[sd]; d.upts[sd] = dints + off_pts[sd]; d.cnt[sd] = dints + off_cnt[sd];
    d.rank[sd] = from_sparse ? dints + off_rank[sd] : nullptr;
    for (int j = 0; j < k; ++j)
      if ((active >> j) & 1ull) { d.mpos[sd][j] = dints + off_mpos[sd][j]; d.feat[sd][j] = dints + off_feat[sd][j]; }
  }
  hipError_t e = hipMemcpyAsync(dmeta, meta.data(), meta.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(sil, 0, sil_dbl * sizeof(double), h->stream);
  if (e == hipSuccess) e = bisil_enqueue_sides(h, vs, k, metric, from_sparse, active, n_u, cnt, plan, d, buf, sil);
  if (e == hipSuccess) e = hipMemcpyAsync(row_sil, sil, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(col_sil, sil + (size_t)n * k, (size_t)m * k * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return h->fail_hip("bisil", e);
  return RESNMTF_OK;
}
}  // namespace

int resnmtf_bisil(resnmtf_handle* h, int v, int k, const double* row_clusters, const double* col_clusters, int metric,
                  double* row_sil, double* col_sil) {
  return bisil_impl(h, v, k, row_clusters, col_clusters, metric, row_sil, col_sil, false);
}

int resnmtf_bisil_sparse(resnmtf_handle* h, int v, int k, const double* row_clusters, const double* col_clusters, int metric,
                         double* row_sil, double* col_sil) {
  return bisil_impl(h, v, k, row_clusters, col_clusters, metric, row_sil, col_sil, true);
}

// The same from 0 / 1 matrices that are ALREADY in device memory, with the silhouettes left there and the view's score
// combined there (resnmtf_bisil.hip.inc).  Dense and sparse views alike: G is gathered or scattered
// as the view is stored.  The lists bisil_impl builds on the host are built by kernels, in its order, so the silhouettes
// are its bits; the host reads back 2 k + 3 ints -- the refusal bits, |U| of both sides and the 2 k member counts -- to
// size the grids and the workspace (bisil_plan), and at the end the score.
// Transient device memory, beyond the workspace of resnmtf_bisil: the two u64 arrays (membership words, umask) and the
// int arrays upts and (sparse) rank over n + m points, the lists mpos_j and feat_j and the gathered member silhouettes
// over sum |I_j| + sum |J_j| entries: O(n + m + sum |I_j| + sum |J_j|).
int resnmtf_bisil_device(resnmtf_handle* h, int v, int k, const resnmtf_device_matrix* row_clusters,
                         const resnmtf_device_matrix* col_clusters, int metric, double* row_sil, double* col_sil,
                         double* view_score, void* stream) {
  if (int rc = check_view(h, v)) return rc;
  if (!row_clusters || !col_clusters || !row_clusters->ptr || !col_clusters->ptr || !view_score)
    return h->fail(RESNMTF_ERR_INVALID, "row_clusters / col_clusters / view_score are NULL");
  if (k < 1 || k > RESNMTF_MAX_K) return h->fail(RESNMTF_ERR_INVALID, "k must be in [1, 64]");
  if (metric < BISIL_EUCLIDEAN || metric > BISIL_COSINE)
    return h->fail(RESNMTF_ERR_INVALID, "metric must be 0 (euclidean), 1 (manhattan) or 2 (cosine)");
  for (const resnmtf_device_matrix* a : {row_clusters, col_clusters}) {
    if (a->dtype != RESNMTF_DTYPE_F64 && a->dtype != RESNMTF_DTYPE_F32 && a->dtype != RESNMTF_DTYPE_F16 && a->dtype != RESNMTF_DTYPE_BF16)
      return h->fail(RESNMTF_ERR_INVALID, "unknown dtype: one of RESNMTF_DTYPE_F64 / _F32 / _F16 / _BF16");
    if (a->row_stride < 0 || a->col_stride < 0) return h->fail(RESNMTF_ERR_INVALID, "negative strides are not supported");
  }
  for (const resnmtf_device_matrix* a : {row_clusters, col_clusters})
    if (!on_handle_device(h, a->ptr))
      return h->fail(RESNMTF_ERR_INVALID, "a cluster matrix is not device memory of the handle's device (host matrices: resnmtf_bisil)");
  for (const double* p : {row_sil, col_sil})
    if (p && !on_handle_device(h, p))
      return h->fail(RESNMTF_ERR_INVALID, "row_sil / col_sil are not device memory of the handle's device (host buffers: resnmtf_bisil)");
  const ViewState& vs = h->views[v];
  bool from_sparse = false;
  if (int rc = bisil_check_state(h, vs, true, &from_sparse)) return rc;
  const int n = vs.n, m = vs.m;
  const size_t pts = (size_t)n + m, sil_dbl = (size_t)n * k + (size_t)m * k;
  const int n_hdr = BISIL_HDR_COUNTS + 2 * k;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  Scratch sc;                             // (dies after the last synchronisation below)
  // [words n + m][umask n + m] u64 | [upts n + m][(sparse) rank n + m][hdr] ints
  const size_t pre_ints = pts * (from_sparse ? 2 : 1) + n_hdr;
  char* pre = sc.take<char>(2 * pts * sizeof(unsigned long long) + pre_ints * sizeof(int));
  if (!pre) return h->fail_hip("hipMalloc bisil_device metadata", sc.error());
  unsigned long long *words = reinterpret_cast<unsigned long long*>(pre), *umask = words + pts;
  int* upts = reinterpret_cast<int*>(umask + pts);
  int* rank = from_sparse ? upts + pts : nullptr;
  int* hdr = upts + pts * (from_sparse ? 2 : 1);
  std::vector<int> hdr_host(n_hdr, 0);
  hipError_t e = wait_for_caller(h, stream);
  if (e == hipSuccess) e = hipMemsetAsync(hdr, 0, (size_t)n_hdr * sizeof(int), h->stream);
  if (e == hipSuccess) {
    auto pack = [&](const resnmtf_device_matrix* a, int len, int bad_bit, unsigned long long* w, int* count) {
      pick_int<RESNMTF_DTYPE_F64, RESNMTF_DTYPE_F32, RESNMTF_DTYPE_F16, RESNMTF_DTYPE_BF16>(a->dtype, [&](auto dt) {
        pick_bools([&](auto along_r) {
          hipLaunchKernelGGL((bisil_words_kernel<decltype(dt)::value, decltype(along_r)::value>), dim3((unsigned)ceil_div(len, 256)), dim3(256), 0,
                             h->stream, a->ptr, a->row_stride, a->col_stride, len, k, bad_bit, w, count, hdr);
        }, a->row_stride < a->col_stride);
      });
    };
    pack(row_clusters, n, 1, words, hdr + BISIL_HDR_COUNTS);
    pack(col_clusters, m, 2, words + n, hdr + BISIL_HDR_COUNTS + k);
    const BisilSideMeta sr = {words, n, umask, upts, rank}, scl = {words + n, m, umask + n, upts + n, rank ? rank + n : nullptr};
    hipLaunchKernelGGL(bisil_union_kernel<0>, dim3(2), dim3(BISIL_SCAN_THREADS), 0, h->stream, sr, scl, k, hdr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hdr_host.data(), hdr, (size_t)n_hdr * sizeof(int), hipMemcpyDeviceToHost, h->stream);
  {
    const hipError_t es = hipStreamSynchronize(h->stream);   // the one read-back
    if (e == hipSuccess) e = es;
  }
  if (e != hipSuccess) return h->fail_hip("bisil_device (metadata)", e);
  if (hdr_host[0])
    return h->fail(RESNMTF_ERR_INVALID, (hdr_host[0] & 1) ? "row_clusters entries must be 0 or 1" : "col_clusters entries must be 0 or 1");
  const int n_u[2] = {hdr_host[1], hdr_host[2]};
  const int* const cnt[2] = {hdr_host.data() + BISIL_HDR_COUNTS, hdr_host.data() + BISIL_HDR_COUNTS + k};
  unsigned long long active = 0ull;                            // biclusters with rows and columns
  for (int j = 0; j < k; ++j) if (cnt[0][j] > 0 && cnt[1][j] > 0) active |= 1ull << j;
  if (!active) {
    if (row_sil) e = hipMemsetAsync(row_sil, 0, (size_t)n * k * sizeof(double), h->stream);
    if (e == hipSuccess && col_sil) e = hipMemsetAsync(col_sil, 0, (size_t)m * k * sizeof(double), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return h->fail_hip("bisil_device", e);
    *view_score = 0.0;
    return RESNMTF_OK;
  }
  BisilPlan plan;
  bisil_plan(k, active, n_u, cnt, plan);
  // the lists of every active bicluster: per side mpos_j then feat_j (ints), and the members' silhouettes (doubles)
  BisilOffsets off = {};
  size_t n_ints = 0, n_vals = 0;
  for (int sd = 0; sd < 2; ++sd)
    for (int j = 0; j < k; ++j) {
      if (!((active >> j) & 1ull)) continue;
      off.mpos[sd][j] = (int)n_ints; n_ints += cnt[sd][j];
      off.feat[sd][j] = (int)n_ints; n_ints += cnt[1 - sd][j];
      off.val[sd][j] = (int)n_vals; n_vals += cnt[sd][j];
    }
  if (n_ints > 2147483647u) return h->fail(RESNMTF_ERR_INVALID, "the member lists exceed 2^31 - 1 entries");
  // [G | norm2 | partial (BisilPlan::work_dbl)][sil n k + m k][vals][means 2 x 64][score] doubles | [lists] ints
  const size_t n_dbl = plan.work_dbl() + sil_dbl + n_vals + 2 * RESNMTF_MAX_K + 1;
  const size_t bytes = n_dbl * sizeof(double) + n_ints * sizeof(int);
  char* buf = nullptr;
  if (int rc = bisil_take_workspace(h, sc, bytes, plan.g_floats, &buf)) return rc;
  double* sil = reinterpret_cast<double*>(buf) + plan.work_dbl();
  double *vals = sil + sil_dbl, *means = vals + n_vals, *score = means + 2 * RESNMTF_MAX_K;
  int* lists = reinterpret_cast<int*>(score + 1);
  BisilLists d;
  for (int sd = 0; sd < 2; ++sd) {
    d.umask[sd] = umask + (sd ? n : 0); d.upts[sd] = upts + (sd ? n : 0); d.cnt[sd] = hdr + BISIL_HDR_COUNTS + sd * k;
    d.rank[sd] = rank ? rank + (sd ? n : 0) : nullptr;
    for (int j = 0; j < k; ++j)
      if ((active >> j) & 1ull) { d.mpos[sd][j] = lists + off.mpos[sd][j]; d.feat[sd][j] = lists + off.feat[sd][j]; }
  }
  e = hipMemsetAsync(sil, 0, sil_dbl * sizeof(double), h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(bisil_members_kernel<0>, dim3(k, 2), dim3(BISIL_SCAN_THREADS), 0, h->stream, d.umask[0], d.upts[0], n_u[0],
                       d.umask[1], d.upts[1], n_u[1], active, off, lists);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bisil_enqueue_sides(h, vs, k, metric, from_sparse, active, n_u, cnt, plan, d, buf, sil);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(bisil_member_mean_kernel<0>, dim3(k, 2), dim3(256), 0, h->stream, (const double*)sil, n, m, k,
                       (const int*)(hdr + BISIL_HDR_COUNTS), active, off, (const int*)lists, vals, means);
    hipLaunchKernelGGL(bisil_score_kernel<0>, dim3(1), dim3(64), 0, h->stream, (const double*)means, k, active, score);
    e = hipGetLastError();
  }
  double score_host = 0.0;
  if (e == hipSuccess && row_sil) e = hipMemcpyAsync(row_sil, sil, (size_t)n * k * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess && col_sil) e = hipMemcpyAsync(col_sil, sil + (size_t)n * k, (size_t)m * k * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&score_host, score, sizeof(double), hipMemcpyDeviceToHost, h->stream);
  {
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = es;
  }
  if (e != hipSuccess) return h->fail_hip("bisil_device", e);
  *view_score = score_host;
  return RESNMTF_OK;
}

namespace {
// The JSD pipeline, enqueued on `st`: the n_cols columns of `cols` ([n_cols][n]) sorted (tiles in sort_a, then merge passes
// between sort_a and sort_b), the statistics of every column, then out[p] for the n_pairs column pairs of `pairs`, in grids
// of at most 2^20 workgroups.  `dens` (nullable): [n_pairs][2][512], the pair kernel's densities.  Returns the buffer the
// statistics and pair kernels read (the last merge destination: sort_a or sort_b).  All pointers are device memory; the
// caller checks hipGetLastError.
const double* enqueue_jsd(hipStream_t st, const double* cols, int n, int n_cols, double* sort_a, double* sort_b, double* stats,
                          const int* pairs, long long n_pairs, double* out, double* dens) {
  hipLaunchKernelGGL(jsd_tile_sort_kernel, dim3(ceil_div(n, JSD_TILE), (unsigned)n_cols), dim3(JSD_SORT_THREADS), 0, st, cols, sort_a, n);
  double *src = sort_a, *dst = sort_b;
  for (int width = JSD_TILE; width < n; width *= 2) {
    hipLaunchKernelGGL(jsd_merge_kernel, dim3(ceil_div(n, 256), (unsigned)n_cols), dim3(256), 0, st, (const double*)src, dst, n, width);
    std::swap(src, dst);
  }
  hipLaunchKernelGGL(jsd_stats_kernel, dim3((unsigned)n_cols), dim3(256), 0, st, (const double*)src, cols, n, std::pow((double)n, -0.2),
                     stats);
  for (long long p0 = 0; p0 < n_pairs; p0 += 1 << 20)
    hipLaunchKernelGGL(jsd_pair_kernel, dim3((unsigned)std::min<long long>(1 << 20, n_pairs - p0)), dim3(JSD_N), 0, st, (const double*)src,
                       (const double*)stats, n, pairs + 2 * (size_t)p0, out + p0, dens ? dens + 2 * (size_t)JSD_N * (size_t)p0 : nullptr);
  return src;
}
}  // namespace

int resnmtf_jsd_stages(int device_id, int n, int n_cols, const double* cols, int n_pairs, const int* pairs, double* out,
                       double* sorted, double* stats_out, double* dens) {
  auto bad = [](const char* msg) { g_create_error = msg; return RESNMTF_ERR_INVALID; };
  if (n < 2) return bad("n must be at least 2 (bw.nrd0 needs two data points)");
  if (n_cols < 1 || n_cols > 65535 || n_pairs < 0) return bad("n_cols must be in [1, 65535] and n_pairs non-negative");
  if (!cols || !pairs || !out) return bad("cols / pairs / out are NULL");
  if ((size_t)n * (size_t)n_cols > ((size_t)1 << 31)) return bad("n * n_cols exceeds 2^31 entries");
  const size_t total = (size_t)n * n_cols;
  for (size_t i = 0; i < total; ++i)
    if (!std::isfinite(cols[i])) return bad("cols has a non-finite entry");
  for (int p = 0; p < 2 * n_pairs; ++p)
    if (pairs[p] < 0 || pairs[p] >= n_cols) return bad("pair index out of range");
  if (n_pairs == 0 && !sorted && !stats_out) return RESNMTF_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_error = "no HIP device"; return RESNMTF_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return bad("device_id out of range");
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  hipStream_t st = nullptr;
  e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  // [orig n C][sort A n C][sort B n C][stats 2 C][out P][dens 1024 P, when asked for] doubles | [pairs 2 P] ints
  const size_t n_dens = dens ? 2 * (size_t)JSD_N * (size_t)n_pairs : 0;
  const size_t n_dbl = 3 * total + 2 * (size_t)n_cols + (size_t)n_pairs + n_dens;
  Scratch sc;
  char* buf = sc.take<char>(n_dbl * sizeof(double) + 2 * (size_t)n_pairs * sizeof(int));
  e = sc.error();
  if (e != hipSuccess) {
    (void)hipStreamDestroy(st);
    g_create_error = std::string("jsd_pairs: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  double *orig = reinterpret_cast<double*>(buf), *sa = orig + total, *sb = sa + total, *stats = sb + total;
  double* dout = stats + 2 * (size_t)n_cols;
  double* ddens = dens ? dout + n_pairs : nullptr;
  int* dpairs = reinterpret_cast<int*>(buf + n_dbl * sizeof(double));
  const double* dsorted = nullptr;
  e = hipMemcpyAsync(orig, cols, total * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_pairs > 0) e = hipMemcpyAsync(dpairs, pairs, 2 * (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    dsorted = enqueue_jsd(st, orig, n, n_cols, sa, sb, stats, dpairs, n_pairs, dout, ddens);
    e = hipGetLastError();
  }
  if (e == hipSuccess && n_pairs > 0) e = hipMemcpyAsync(out, dout, (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && sorted) e = hipMemcpyAsync(sorted, dsorted, total * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && stats_out) e = hipMemcpyAsync(stats_out, stats, 2 * (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_dens) e = hipMemcpyAsync(dens, ddens, n_dens * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipStreamDestroy(st);
  if (e != hipSuccess) { g_create_error = std::string("jsd_pairs: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  return RESNMTF_OK;
}

int resnmtf_jsd_pairs(int device_id, int n, int n_cols, const double* cols, int n_pairs, const int* pairs, double* out) {
  return resnmtf_jsd_stages(device_id, n, n_cols, cols, n_pairs, pairs, out, nullptr, nullptr, nullptr);
}

// ---- spurious-bicluster scoring of handles (check_biclusters with get_thresholds, R/obtain_bicl.r:80-133): the pool
// cbind(F_v, f_1, ..., f_R) gathered on the device from the handles' own F, then resnmtf_jsd_pairs' kernels over
// pool_pairs(K, R) (resnmtf_amd/spurious.py), the K means on the device
int resnmtf_spurious_scores(resnmtf_handle* h, int v, resnmtf_handle* const* shuffles, int R, double* score,
                            double* null_scores) {
  if (int rc = check_view(h, v)) return rc;
  if (!shuffles || !score || !null_scores) return h->fail(RESNMTF_ERR_INVALID, "shuffles / score / null_scores are NULL");
  if (R < 2) return h->fail(RESNMTF_ERR_INVALID, "R must be at least 2 (the reference indexes a second shuffled repeat)");
  const ViewState& vs = h->views[v];
  const int n = vs.n, K = vs.k;
  if (!vs.has_factors) return h->fail(RESNMTF_ERR_STATE, "the view has no factors");
  if (n < 2) return h->fail(RESNMTF_ERR_INVALID, "n must be at least 2 (bw.nrd0 needs two data points)");
  for (int r = 0; r < R; ++r) {
    const resnmtf_handle* s = shuffles[r];
    if (!s) return h->fail(RESNMTF_ERR_INVALID, "a shuffle handle is NULL");
    if (v >= s->V) return h->fail(RESNMTF_ERR_INVALID, "a shuffle handle has no view v");
    if (s->opt.device_id != h->opt.device_id) return h->fail(RESNMTF_ERR_INVALID, "handles live on different devices");
    if (s->views[v].n != n || s->views[v].k != K) return h->fail(RESNMTF_ERR_INVALID, "a shuffle handle's view v differs in n or k");
    if (!s->views[v].has_factors) return h->fail(RESNMTF_ERR_STATE, "a shuffle handle's view v has no factors");
  }
  const long long C = (long long)K * (R + 1);
  const long long RK = (long long)R * K;
  const long long P_null = (long long)K * K * R * (R - 1) / 2, P = P_null + (long long)K * RK;
  if (C > 65535) return h->fail(RESNMTF_ERR_INVALID, "K (R + 1) exceeds 65535 pool columns");
  if ((long long)n * C > ((long long)1 << 31)) return h->fail(RESNMTF_ERR_INVALID, "n K (R + 1) exceeds 2^31 entries");
  if (P > 2147483647LL) return h->fail(RESNMTF_ERR_INVALID, "K^2 R (R + 1) / 2 pairs exceed 2^31 - 1");
  // the pairs in pool_pairs' order: null (calculate_f_shuffle_jsd, :55-68), then score (check_biclusters, :125-128)
  std::vector<int> pairs(2 * (size_t)P);
  size_t q = 0;
  for (int j = 0; j < R - 1; ++j)
    for (int k = 0; k < K; ++k)
      for (int l = j + 1; l < R; ++l)
        for (int m = 0; m < K; ++m) { pairs[q++] = K + j * K + k; pairs[q++] = K + l * K + m; }
  for (int k = 0; k < K; ++k)
    for (int y = 0; y < R * K; ++y) { pairs[q++] = k; pairs[q++] = K + y; }
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  for (int r = 0; r < R; ++r) HIP_TRY(h, hipStreamSynchronize(shuffles[r]->stream));
  const size_t total = (size_t)n * C, nk = (size_t)n * K;
  // [pool n C][sort A n C][sort B n C][stats 2 C][colsum K][clusters n K (unused)][out P][score K] doubles
  // | [pairs 2 P][flag 1] ints
  const size_t n_dbl = 3 * total + 2 * (size_t)C + (size_t)K + nk + (size_t)P + (size_t)K;
  Scratch sc;
  char* buf = sc.take<char>(n_dbl * sizeof(double) + (2 * (size_t)P + 1) * sizeof(int));
  if (!buf) return h->fail_hip("spurious_scores hipMalloc", sc.error());
  double *pool = reinterpret_cast<double*>(buf), *sa = pool + total, *sb = sa + total, *stats = sb + total;
  double *cF = stats + 2 * (size_t)C, *cl = cF + K, *dout = cl + nk, *dscore = dout + P;
  int* dpairs = reinterpret_cast<int*>(buf + n_dbl * sizeof(double));
  int* dflag = dpairs + 2 * (size_t)P;
  int flag = 0;
  hipError_t e = hipMemcpyAsync(dpairs, pairs.data(), 2 * (size_t)P * sizeof(int), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(dflag, 0, sizeof(int), h->stream);
  if (e == hipSuccess) {
    // F / colSums(F) of every handle, as resnmtf_finalise computes it (same kernels), into its K pool columns
    for (int t = 0; t <= R; ++t) {
      const ViewState& src = t == 0 ? vs : shuffles[t - 1]->views[v];
      hipLaunchKernelGGL(colsum_kernel, dim3(K), dim3(256), 0, h->stream, (const double*)src.side[SIDE_F].W, n, K, cF);
      hipLaunchKernelGGL(finalise_factor_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream,
                         (const double*)src.side[SIDE_F].W, n, K, (const double*)cF, (const int*)nullptr, pool + (size_t)t * nk, cl);
    }
    hipLaunchKernelGGL(jsd_finite_kernel, dim3((unsigned)std::min<size_t>(1024, (total + 255) / 256)), dim3(256), 0,
                       h->stream, (const double*)pool, total, dflag);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess && flag) return h->fail(RESNMTF_ERR_INVALID, "a factor has a non-finite entry");
  if (e == hipSuccess) {
    enqueue_jsd(h->stream, pool, n, (int)C, sa, sb, stats, dpairs, P, dout, nullptr);
    hipLaunchKernelGGL(jsd_score_mean_kernel, dim3((unsigned)ceil_div(K, 64)), dim3(64), 0, h->stream,
                       (const double*)(dout + P_null), K, (int)RK, dscore);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(score, dscore, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(null_scores, dout, (size_t)P_null * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return h->fail_hip("spurious_scores", e);
  return RESNMTF_OK;
}

// ---- grouped small factorisations (csrc/resnmtf_group.hip.inc) ----
namespace {
bool all_finite(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// what an entry point that takes a resnmtf_group_job allows: resnmtf_group_run (one workgroup per job) and
// resnmtf_fp64_run (device-wide) share every check below and differ in these
struct GroupJobLimits {
  int max_k;
  const char* k_text;
  long long max_view_entries;            // 0 = no cap on n * m
};
const GroupJobLimits kGroupLimits = {RESNMTF_GROUP_MAX_K, "k must be in [1, 32]", RESNMTF_GROUP_MAX_VIEW_ENTRIES};
const GroupJobLimits kFp64Limits = {RESNMTF_MAX_K, "k must be in [1, 64]", 0};

// a job's host checks; a message on refusal, nullptr when it is fine
// (x_elsewhere: bit v set = view v's data come from outside the job, resnmtf_fp64_run_sparse's CSC arrays or
// resnmtf_fp64_run_device's device matrix, and x[v] must be NULL; factors_elsewhere: bit v set = so do its initial factors,
// and f0 / s0 / g0 / lambda0 / mu0 [v] must be NULL; outputs_elsewhere: the results go to device memory and the job's five
// output pointers per view may be NULL)
const char* check_group_job(const resnmtf_group_job& j, int max_iters, const GroupJobLimits& lim, unsigned x_elsewhere = 0,
                            unsigned factors_elsewhere = 0, bool outputs_elsewhere = false) {
  if (j.struct_size != (int)sizeof(resnmtf_group_job)) return "resnmtf_group_job struct_size mismatch";
  const int V = j.n_views, k = j.k;
  if (V < 1 || V > RESNMTF_GROUP_MAX_VIEWS) return "n_views must be in [1, 8]";
  if (k < 1 || k > lim.max_k) return lim.k_text;
  if (j.n_iters < 0) return "n_iters must be >= 0 (0 = run to convergence)";
  const int sweeps = j.n_iters > 0 ? std::min(j.n_iters, max_iters) : max_iters;
  if (!j.all_error || !j.iters_done || j.err_capacity < sweeps) return "all_error / iters_done NULL or err_capacity below the sweeps allowed";
  for (int v = 0; v < V; ++v) {
    const int n = j.n_rows[v], m = j.n_cols[v];
    if (n < 1 || m < 1) return "view dimensions must be positive";
    if (k > n || k > m) return "k exceeds a view dimension (R/utils.r:444,449)";
    if (lim.max_view_entries > 0 && (long long)n * m > lim.max_view_entries) return "a view has more than 2^22 entries";
    const bool elsewhere = (x_elsewhere >> v) & 1u;
    if (elsewhere && j.x[v]) return "a view is given both dense (x) and sparse (col_ptr): x must be NULL for a sparse view";
    const bool factors_there = (factors_elsewhere >> v) & 1u;
    if (factors_there && (j.f0[v] || j.s0[v] || j.g0[v] || j.lambda0[v] || j.mu0[v]))
      return "a view's initial factors are given in device memory: f0 / s0 / g0 / lambda0 / mu0 must be NULL for it";
    if ((!elsewhere && !j.x[v]) || (!factors_there && (!j.f0[v] || !j.s0[v] || !j.g0[v]))) return "x / f0 / s0 / g0 is NULL";
    if (!outputs_elsewhere && (!j.f_out[v] || !j.s_out[v] || !j.g_out[v] || !j.lambda_out[v] || !j.mu_out[v]))
      return "an output pointer is NULL";
    if (!elsewhere && !all_finite(j.x[v], (size_t)n * m)) return "x has a non-finite entry";
    if (factors_there) continue;
    if (!all_finite(j.f0[v], (size_t)n * k) || !all_finite(j.s0[v], (size_t)k * k) || !all_finite(j.g0[v], (size_t)m * k))
      return "an initial factor has a non-finite entry";
    if ((j.lambda0[v] && !all_finite(j.lambda0[v], k)) || (j.mu0[v] && !all_finite(j.mu0[v], k)))
      return "lambda0 / mu0 has a non-finite entry";
  }
  for (const double* r : {j.phi, j.xi, j.psi}) {
    if (!r) continue;
    for (int w = 0; w < V; ++w)
      for (int v = 0; v < V; ++v) {
        const double x = r[w + v * V];
        if (!std::isfinite(x) || x < 0) return "restriction entries must be finite and non-negative";
        if (v == w && x != 0) return "restriction matrices must have a zero diagonal (init_rest_mats)";
      }
  }
  for (int v = 0; v < V; ++v)
    for (int w = 0; w < V; ++w) {
      if (v == w) continue;
      for (int axis = 0; axis < 2; ++axis) {
        const int c = axis ? j.col_count[v][w] : j.row_count[v][w];
        if (c <= 0) continue;
        const int* iv = axis ? j.col_idx_v[v][w] : j.row_idx_v[v][w];
        const int* iw = axis ? j.col_idx_w[v][w] : j.row_idx_w[v][w];
        const int lv = axis ? j.n_cols[v] : j.n_rows[v], lw = axis ? j.n_cols[w] : j.n_rows[w];
        if (!iv || !iw) return "shared index arrays are NULL";
        for (int p = 0; p < c; ++p)
          if (iv[p] < 0 || iv[p] >= lv || iw[p] < 0 || iw[p] >= lw) return "shared index out of range";
      }
    }
  return nullptr;
}
}  // namespace

int resnmtf_group_run(int device_id, int n_jobs, const resnmtf_group_job* jobs, double tol, int max_iters) {
  auto bad = [](const std::string& msg) { g_create_error = msg; return RESNMTF_ERR_INVALID; };
  if (n_jobs < 0) return bad("n_jobs must be >= 0");
  if (n_jobs > 0 && !jobs) return bad("jobs is NULL");
  if (max_iters < 1) return bad("max_iters must be >= 1");
  if (!std::isfinite(tol)) return bad("tol must be finite");
  for (int q = 0; q < n_jobs; ++q)
    if (const char* why = check_group_job(jobs[q], max_iters, kGroupLimits)) return bad("job " + std::to_string(q) + ": " + why);
  if (n_jobs == 0) return RESNMTF_OK;

  // one buffer: [descriptors | outputs (F, G, S, lambda, mu per job) | sweep counts | X, X^T | row / column maps |
  // error histories | scratch]; everything before the error histories is uploaded; the outputs and sweep counts come
  // back, then the first max(sweeps) rows of the error histories (sweep-major: entry it * n_jobs + job)
  std::vector<GroupDesc> desc(n_jobs);
  size_t off = ((size_t)n_jobs * sizeof(GroupDesc) + 15) / 16 * 2;      // in doubles
  int lds[3] = {0, 0, 0};                                                 // per k class (8, 16, 32)
  int max_cap = 1;
  for (int q = 0; q < n_jobs; ++q) {
    const resnmtf_group_job& j = jobs[q];
    GroupDesc& d = desc[q];
    std::memset(&d, 0, sizeof(d));
    d.V = j.n_views; d.k = j.k; d.n_iters = j.n_iters; d.id = q;
    d.cap = j.n_iters > 0 ? std::min(j.n_iters, max_iters) : max_iters;
    d.tol = tol;
    for (int v = 0; v < d.V; ++v) {
      d.n[v] = j.n_rows[v]; d.m[v] = j.n_cols[v];
      d.f[v] = off; off += (size_t)d.n[v] * d.k;
      d.g[v] = off; off += (size_t)d.m[v] * d.k;
    }
    d.s = off; off += (size_t)d.V * d.k * d.k;
    d.lam = off; off += (size_t)d.V * d.k;
    d.mu = off; off += (size_t)d.V * d.k;
    max_cap = std::max(max_cap, d.cap);
    for (int w = 0; w < d.V; ++w)
      for (int v = 0; v < d.V; ++v) {
        d.phi[w * GRP_MAX_VIEWS + v] = j.phi ? j.phi[w + v * d.V] : 0.0;
        d.xi[w * GRP_MAX_VIEWS + v] = j.xi ? j.xi[w + v * d.V] : 0.0;
        d.psi[w * GRP_MAX_VIEWS + v] = j.psi ? j.psi[w + v * d.V] : 0.0;
      }
    const int cls = d.k <= 8 ? 0 : (d.k <= 16 ? 1 : 2);
    lds[cls] = std::max(lds[cls], group_lds_doubles(d.V, d.k));
  }
  const size_t sweeps_off = off;                                          // n_jobs ints, padded to doubles
  off += ((size_t)n_jobs + 1) / 2;
  const size_t upload_x = off;
  for (int q = 0; q < n_jobs; ++q) {
    GroupDesc& d = desc[q];
    for (int v = 0; v < d.V; ++v) {
      d.x[v] = off; off += (size_t)d.n[v] * d.m[v];
      d.xt[v] = off; off += (size_t)d.n[v] * d.m[v];
    }
  }
  size_t ioff = off * 2;                                                  // maps, in ints from the buffer base
  for (int q = 0; q < n_jobs; ++q) {
    const resnmtf_group_job& j = jobs[q];
    GroupDesc& d = desc[q];
    for (int v = 0; v < GRP_MAX_VIEWS; ++v)
      for (int w = 0; w < GRP_MAX_VIEWS; ++w) {
        const bool pair = v < d.V && w < d.V && v != w;
        d.rmap[v][w] = pair && j.row_count[v][w] > 0 ? (long long)ioff : -1;
        if (d.rmap[v][w] >= 0) ioff += d.n[v];
        d.cmap[v][w] = pair && j.col_count[v][w] > 0 ? (long long)ioff : -1;
        if (d.cmap[v][w] >= 0) ioff += d.m[v];
      }
  }
  off = (ioff + 1) / 2;
  const size_t upload_end = off;
  const size_t err_base = off;
  off += (size_t)n_jobs * max_cap;
  for (int q = 0; q < n_jobs; ++q) { desc[q].err = (long long)(err_base + q); desc[q].err_stride = n_jobs; }
  for (int q = 0; q < n_jobs; ++q) {
    GroupDesc& d = desc[q];
    int big = 1;
    for (int v = 0; v < d.V; ++v) big = std::max(big, std::max(d.n[v], d.m[v]));
    d.scratch = off; off += (size_t)big * d.k;
    d.scratch2 = off; off += (size_t)big * d.k;
  }
  const size_t total = off;

  // descriptors grouped by k class (stable), one launch per class
  std::vector<GroupDesc> sorted;
  int class_first[4] = {0, 0, 0, 0};
  const int classes[3] = {8, 16, 32};
  for (int c = 0; c < 3; ++c) {
    class_first[c] = (int)sorted.size();
    for (int q = 0; q < n_jobs; ++q)
      if (group_k_class(desc[q].k) == classes[c]) sorted.push_back(desc[q]);
  }
  class_first[3] = n_jobs;
  std::vector<double> host(upload_end, 0.0);
  std::memcpy(host.data(), sorted.data(), (size_t)n_jobs * sizeof(GroupDesc));
  int* ihost = reinterpret_cast<int*>(host.data());
  for (int q = 0; q < n_jobs; ++q) {
    const resnmtf_group_job& j = jobs[q];
    const GroupDesc& d = desc[q];
    const int k = d.k;
    for (int v = 0; v < d.V; ++v) {
      const int n = d.n[v], m = d.m[v];
      std::memcpy(&host[d.f[v]], j.f0[v], (size_t)n * k * sizeof(double));
      std::memcpy(&host[d.g[v]], j.g0[v], (size_t)m * k * sizeof(double));
      std::memcpy(&host[d.s + (size_t)v * k * k], j.s0[v], (size_t)k * k * sizeof(double));
      for (int c = 0; c < k; ++c) {                                       // explicit init: colSums (R/update_steps.r:55-56)
        double cf = 0.0, cg = 0.0;
        if (!j.lambda0[v]) for (int i = 0; i < n; ++i) cf += j.f0[v][i + (size_t)c * n];
        if (!j.mu0[v]) for (int i = 0; i < m; ++i) cg += j.g0[v][i + (size_t)c * m];
        host[d.lam + (size_t)v * k + c] = j.lambda0[v] ? j.lambda0[v][c] : cf;
        host[d.mu + (size_t)v * k + c] = j.mu0[v] ? j.mu0[v][c] : cg;
      }
      const double* x = j.x[v];
      std::memcpy(&host[d.x[v]], x, (size_t)n * m * sizeof(double));
      double* xt = &host[d.xt[v]];
      for (int c = 0; c < m; ++c)
        for (int i = 0; i < n; ++i) xt[c + (size_t)i * m] = x[i + (size_t)c * n];
      for (int w = 0; w < d.V; ++w) {
        if (d.rmap[v][w] >= 0) {
          int* map = ihost + d.rmap[v][w];
          std::fill(map, map + n, -1);
          for (int p = 0; p < j.row_count[v][w]; ++p) map[j.row_idx_v[v][w][p]] = j.row_idx_w[v][w][p];
        }
        if (d.cmap[v][w] >= 0) {
          int* map = ihost + d.cmap[v][w];
          std::fill(map, map + m, -1);
          for (int p = 0; p < j.col_count[v][w]; ++p) map[j.col_idx_v[v][w][p]] = j.col_idx_w[v][w][p];
        }
      }
    }
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_error = "no HIP device"; return RESNMTF_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return bad("device_id out of range");
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  const size_t lds_bytes[3] = {(size_t)lds[0] * sizeof(double), (size_t)lds[1] * sizeof(double), (size_t)lds[2] * sizeof(double)};
  e = hipSuccess;
  if (lds[0] > 0) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&group_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes[0]);
  if (e == hipSuccess && lds[1] > 0) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&group_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes[1]);
  if (e == hipSuccess && lds[2] > 0) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&group_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes[2]);
  if (e != hipSuccess) { g_create_error = std::string("group_run: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  hipStream_t st = nullptr;
  e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  Scratch sc;
  double* buf = sc.take<double>(total);
  e = sc.error();
  if (e != hipSuccess) {
    (void)hipStreamDestroy(st);
    g_create_error = std::string("group_run: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  const size_t desc_dbl = ((size_t)n_jobs * sizeof(GroupDesc) + 15) / 16 * 2;
  e = hipMemcpyAsync(buf, host.data(), upload_end * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const GroupDesc* dd = reinterpret_cast<const GroupDesc*>(buf);
    int* dsweeps = reinterpret_cast<int*>(buf + sweeps_off);
    const int cnt[3] = {class_first[1] - class_first[0], class_first[2] - class_first[1], class_first[3] - class_first[2]};
    if (cnt[0] > 0) hipLaunchKernelGGL(group_kernel<8>, dim3(cnt[0]), dim3(GRP_THREADS), lds_bytes[0], st, dd + class_first[0], buf, (const int*)buf, dsweeps);
    if (cnt[1] > 0) hipLaunchKernelGGL(group_kernel<16>, dim3(cnt[1]), dim3(GRP_THREADS), lds_bytes[1], st, dd + class_first[1], buf, (const int*)buf, dsweeps);
    if (cnt[2] > 0) hipLaunchKernelGGL(group_kernel<32>, dim3(cnt[2]), dim3(GRP_THREADS), lds_bytes[2], st, dd + class_first[2], buf, (const int*)buf, dsweeps);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(host.data() + desc_dbl, buf + desc_dbl, (upload_x - desc_dbl) * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  const int* sweeps = reinterpret_cast<const int*>(host.data() + sweeps_off);
  int max_it = 0;
  if (e == hipSuccess)
    for (int q = 0; q < n_jobs; ++q) max_it = std::max(max_it, std::min(std::max(sweeps[q], 0), desc[q].cap));
  std::vector<double> errs((size_t)max_it * n_jobs);
  if (e == hipSuccess && max_it > 0)
    e = hipMemcpyAsync(errs.data(), buf + err_base, errs.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipStreamDestroy(st);
  if (e != hipSuccess) { g_create_error = std::string("group_run: ") + hipGetErrorString(e); return RESNMTF_ERR_HIP; }
  for (int q = 0; q < n_jobs; ++q) {
    const resnmtf_group_job& j = jobs[q];
    const GroupDesc& d = desc[q];
    const int k = d.k;
    for (int v = 0; v < d.V; ++v) {
      std::memcpy(j.f_out[v], &host[d.f[v]], (size_t)d.n[v] * k * sizeof(double));
      std::memcpy(j.g_out[v], &host[d.g[v]], (size_t)d.m[v] * k * sizeof(double));
      std::memcpy(j.s_out[v], &host[d.s + (size_t)v * k * k], (size_t)k * k * sizeof(double));
      std::memcpy(j.lambda_out[v], &host[d.lam + (size_t)v * k], (size_t)k * sizeof(double));
      std::memcpy(j.mu_out[v], &host[d.mu + (size_t)v * k], (size_t)k * sizeof(double));
    }
    const int it = std::min(std::max(sweeps[q], 0), d.cap);
    for (int t = 0; t < it; ++t) j.all_error[t] = errs[(size_t)t * n_jobs + q];
    *j.iters_done = it;
  }
  return RESNMTF_OK;
}

// ---- device-wide fp64 factorisation: the entry points live in csrc/resnmtf_fp64.hip (a translation unit of its own,
// so that its kernels sit in a code object of their own); these two hand it the checks and the error text it shares
// with resnmtf_group_run (csrc/resnmtf_internal.h) ----
}  // extern "C"
const char* resnmtf_check_fp64_job(const resnmtf_group_job& j, int max_iters, unsigned x_elsewhere, unsigned factors_elsewhere,
                                   bool outputs_elsewhere) {
  return check_group_job(j, max_iters, kFp64Limits, x_elsewhere, factors_elsewhere, outputs_elsewhere);
}
void resnmtf_set_create_error(const std::string& text) { g_create_error = text; }

// The canonical structure of a sparse view in the caller's device memory, for the fp64 path (resnmtf_internal.h; DESIGN.md
// section 24): resnmtf_set_view_sparse_device's checks and finish_sparse_build's two sorts, into arrays the caller owns.
// Host code only: every kernel launched here is one those two launch.
int resnmtf_sparse_device_canonical(void* stream, resnmtf_sparse_device_build& b, void* (*alloc)(void* ctx, size_t bytes), void* ctx,
                                    std::string& why) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool coo = b.layout == RESNMTF_SPARSE_COO, csc = b.layout == RESNMTF_SPARSE_CSC, i64 = b.index_type == RESNMTF_INDEX_I64;
  const int n = b.n, m = b.m, lines = csc ? m : n;
  const long long nnz = b.nnz;
  unsigned long long host_flags[2] = {kSpdvNone, 0ull};
  auto hip_fail = [&](hipError_t e) { why = hipGetErrorString(e); return (int)RESNMTF_ERR_HIP; };
  // the flags as they are on the device after everything enqueued so far; the refusal, if the word holds one
  auto verdict = [&](const unsigned long long* sorted_keys) -> int {
    hipError_t e = hipMemcpyAsync(host_flags, b.flags, sizeof(host_flags), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e);
    if (host_flags[0] == kSpdvNone) return RESNMTF_OK;
    unsigned long long k = 0;
    if (host_flags[0] >> 56 == SPDV_DUPLICATE) {
      e = hipMemcpy(&k, sorted_keys + (host_flags[0] & ((1ull << 56) - 1ull)), sizeof(k), hipMemcpyDeviceToHost);
      if (e != hipSuccess) return hip_fail(e);
    }
    why = spdv_refusal_text(host_flags[0], csc, nnz, n, k);
    return RESNMTF_ERR_INVALID;
  };
  hipError_t e = hipMemcpyAsync(b.flags, host_flags, sizeof(host_flags), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail(e);
  if (!coo) {                                // the line pointers, judged before any kernel bounds a search by them
    spdv_launch_ptr_check(st, i64, b.ptr_or_rows, lines, nnz, b.flags);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
    if (int rc = verdict(nullptr)) return rc;
  }
  if (nnz == 0) return RESNMTF_OK;
  spdv_launch_entries(st, b.layout, i64, b.dtype, b.ptr_or_rows, b.idx_or_cols, b.values, nnz, n, m, b.key[0], reinterpret_cast<double*>(b.pay[0]),
                      nullptr, b.flags);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
  if (int rc = verdict(nullptr)) return rc;
  const bool presorted = csc && host_flags[1] == 0ull;
  const unsigned grid = (unsigned)((nnz + 255) / 256);
  const unsigned long long count = (unsigned long long)n * m;
  unsigned int end_bit = 1;                  // the bits of n m: every key is < count
  while (end_bit < 64 && ((count - 1) >> end_bit) != 0) ++end_bit;
  rocprim::double_buffer<unsigned long long> kb(b.key[0], b.key[1]);
  rocprim::double_buffer<double> vb(reinterpret_cast<double*>(b.pay[0]), reinterpret_cast<double*>(b.pay[1]));
  rocprim::double_buffer<unsigned long long> kb2(b.key[0], b.key[1]);
  rocprim::double_buffer<long long> pb(b.pay[1], b.pay[2]);
  size_t tmp_bytes = 0, tmp_bytes2 = 0;
  e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, vb, (size_t)nnz, 0u, end_bit, st);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, tmp_bytes2, kb2, pb, (size_t)nnz, 0u, end_bit, st);
  if (e != hipSuccess) return hip_fail(e);
  tmp_bytes = std::max<size_t>(std::max(tmp_bytes, tmp_bytes2), 8);
  void* tmp = alloc(ctx, tmp_bytes);
  if (!tmp) return RESNMTF_ERR_ALLOC;
  // ---- the CSC: the entries sorted by c n + r
  if (!presorted) {
    e = rocprim::radix_sort_pairs(tmp, tmp_bytes, kb, vb, (size_t)nnz, 0u, end_bit, st);
    if (e != hipSuccess) return hip_fail(e);
    if (nnz > 1) {
      hipLaunchKernelGGL(sparse_device_duplicates_kernel, dim3((unsigned)((nnz + 254) / 256)), dim3(256), 0, st, kb.current(), nnz, b.flags);
      if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
      if (int rc = verdict(kb.current())) return rc;
    }
  }
  hipLaunchKernelGGL(sorted_lines_kernel, dim3(grid), dim3(256), 0, st, kb.current(), nnz, (unsigned long long)n, m, b.cptr, b.cidx);
  // ---- the CSR: the CSC positions sorted by r m + c (the values stay where the first sort left them)
  kb2 = rocprim::double_buffer<unsigned long long>(kb.alternate(), kb.current());
  pb = rocprim::double_buffer<long long>(reinterpret_cast<long long*>(vb.alternate()), b.pay[2]);
  hipLaunchKernelGGL(sparse_shuffle_csr_keys_kernel, dim3(grid), dim3(256), 0, st, kb.current(), nnz, n, m, kb2.current(), pb.current());
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
  e = rocprim::radix_sort_pairs(tmp, tmp_bytes, kb2, pb, (size_t)nnz, 0u, end_bit, st);
  if (e != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL(sorted_lines_kernel, dim3(grid), dim3(256), 0, st, kb2.current(), nnz, (unsigned long long)m, n, b.rptr, b.ridx);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
  b.csc_values = vb.current();
  b.csr_perm = pb.current();
  return RESNMTF_OK;
}
extern "C" {

int resnmtf_factor_device_ptr(resnmtf_handle* h, int v, int which, void** ptr, size_t* bytes) {
  if (int rc = check_view(h, v)) return rc;
  if (!ptr || !bytes) return h->fail(RESNMTF_ERR_INVALID, "ptr/bytes are NULL");
  ViewState& vs = h->views[v];
  switch (which) {
    case RESNMTF_FACTOR_F: *ptr = vs.side[SIDE_F].W; *bytes = (size_t)vs.n * vs.k * sizeof(double); break;
    case RESNMTF_FACTOR_G: *ptr = vs.side[SIDE_G].W; *bytes = (size_t)vs.m * vs.k * sizeof(double); break;
    case RESNMTF_FACTOR_S: *ptr = vs.S; *bytes = (size_t)vs.k * vs.k * sizeof(double); break;
    case RESNMTF_FACTOR_FBLOCK:
      if (!vs.side[SIDE_F].xblk) return h->fail(RESNMTF_ERR_STATE, "no F exchange block: create the handle with replicate_f = 1");
      *ptr = vs.side[SIDE_F].xblk; *bytes = vs.side[SIDE_F].xblk_bytes; break;
    case RESNMTF_FACTOR_FBLOCK_ALL:
      if (!h->arena[SIDE_F]) return h->fail(RESNMTF_ERR_STATE, "no F exchange blocks: create the handle with replicate_f = 1");
      *ptr = h->arena[SIDE_F]; *bytes = h->arena_bytes[SIDE_F]; break;
    case RESNMTF_FACTOR_GBLOCK:
      if (!vs.side[SIDE_G].xblk) return h->fail(RESNMTF_ERR_STATE, "no G exchange block: create the handle with replicate_gs = 1");
      *ptr = vs.side[SIDE_G].xblk; *bytes = vs.side[SIDE_G].xblk_bytes; break;
    case RESNMTF_FACTOR_GBLOCK_ALL:
      if (!h->arena[SIDE_G]) return h->fail(RESNMTF_ERR_STATE, "no G exchange blocks: create the handle with replicate_gs = 1");
      *ptr = h->arena[SIDE_G]; *bytes = h->arena_bytes[SIDE_G]; break;
    case RESNMTF_FACTOR_SBLOCK:
      if (!vs.sblk) return h->fail(RESNMTF_ERR_STATE, "no S exchange block: create the handle with replicate_gs = 1");
      *ptr = vs.sblk; *bytes = h->sblk_stride * sizeof(double); break;
    case RESNMTF_FACTOR_SBLOCK_ALL:
      if (h->sblk_embedded) return h->fail(RESNMTF_ERR_STATE, "the S blocks of this handle sit inside the F blocks (RESNMTF_FACTOR_FBLOCK_ALL moves both)");
      if (!h->sblk_arena) return h->fail(RESNMTF_ERR_STATE, "no S exchange blocks: create the handle with replicate_gs = 1");
      *ptr = h->sblk_arena; *bytes = h->sblk_stride * sizeof(double) * h->V; break;
    case RESNMTF_FACTOR_U_SEND: case RESNMTF_FACTOR_U_RECV: case RESNMTF_FACTOR_FNEW_SEND: case RESNMTF_FACTOR_FNEW_RECV:
    case RESNMTF_FACTOR_T_SEND: case RESNMTF_FACTOR_T_RECV: case RESNMTF_FACTOR_GNEW_SEND: case RESNMTF_FACTOR_GNEW_RECV:
    case RESNMTF_FACTOR_F_SLICE: case RESNMTF_FACTOR_G_SLICE: {
      if (!h->sliced) return h->fail(RESNMTF_ERR_STATE, "no slice buffers: create the handle with slice_chains = 1");
      const size_t V = (size_t)h->V;
      const size_t fbytes = V * h->sl_len[SIDE_F] * vs.KP * sizeof(float), gbytes = V * h->sl_len[SIDE_G] * vs.KP * sizeof(float);
      switch (which) {
        case RESNMTF_FACTOR_U_SEND: *ptr = h->p_send[SIDE_F]; *bytes = V * h->p_chunk[SIDE_F]; break;
        case RESNMTF_FACTOR_U_RECV: *ptr = h->p_recv[SIDE_F]; *bytes = V * h->p_chunk[SIDE_F]; break;
        case RESNMTF_FACTOR_T_SEND: *ptr = h->p_send[SIDE_G]; *bytes = V * h->p_chunk[SIDE_G]; break;
        case RESNMTF_FACTOR_T_RECV: *ptr = h->p_recv[SIDE_G]; *bytes = V * h->p_chunk[SIDE_G]; break;
        case RESNMTF_FACTOR_FNEW_SEND: *ptr = h->w_send[SIDE_F]; *bytes = fbytes; break;
        case RESNMTF_FACTOR_FNEW_RECV: *ptr = h->w_recv[SIDE_F]; *bytes = fbytes; break;
        case RESNMTF_FACTOR_GNEW_SEND: *ptr = h->w_send[SIDE_G]; *bytes = gbytes; break;
        case RESNMTF_FACTOR_GNEW_RECV: *ptr = h->w_recv[SIDE_G]; *bytes = gbytes; break;
        default: {
          const int s = which == RESNMTF_FACTOR_F_SLICE ? SIDE_F : SIDE_G;
          const int per = h->sl_len[s], full = vs.side[s].len;
          const int begin = std::min(h->opt.slice_index * per, full), len = std::min(per, full - begin);
          *ptr = vs.side[s].W + (size_t)begin * vs.k; *bytes = (size_t)len * vs.k * sizeof(double);
        }
      }
      break;
    }
    default: return h->fail(RESNMTF_ERR_INVALID, "unknown factor selector");
  }
  return RESNMTF_OK;
}

int resnmtf_set_stop_tolerance(resnmtf_handle* h, double tol) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (tol >= 0.0 && !h->opt.replicate_gs)
    return h->fail(RESNMTF_ERR_STATE, "the phase API's stop test runs in the replicated S chain (replicate_gs / slice_chains); resnmtf_run has its own");
  h->phase_tol = tol >= 0.0 ? tol : -1.0;
  return RESNMTF_OK;
}

int resnmtf_loop_state(resnmtf_handle* h, int* sweeps_done, int* done, int* stop_sweep) {
  if (!h) return RESNMTF_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  SweepCtl c{};
  HIP_TRY(h, hipMemcpy(&c, h->ctl, sizeof(c), hipMemcpyDeviceToHost));
  if (sweeps_done) *sweeps_done = c.sweep;
  if (done) *done = c.done;
  if (stop_sweep) *stop_sweep = c.stop_sweep;
  return RESNMTF_OK;
}

int resnmtf_slice_info(resnmtf_handle* h, int* rows_per_slice, int* cols_per_slice) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (!h->sliced) return h->fail(RESNMTF_ERR_STATE, "not a slice_chains handle");
  if (rows_per_slice) *rows_per_slice = h->sl_len[SIDE_F];
  if (cols_per_slice) *cols_per_slice = h->sl_len[SIDE_G];
  return RESNMTF_OK;
}

// what a rank maps of every other rank: sliced chains -- the four receive buffers and the S block arena; block form -- the
// exchange arenas of the replicated layouts (those the layout has); the arrival counters in both
static void p2p_buffers(resnmtf_handle* h, void* bufs[6]) {
  if (h->block_p2p) {
    bufs[0] = h->arena[SIDE_F]; bufs[1] = nullptr; bufs[2] = h->arena[SIDE_G]; bufs[3] = nullptr; bufs[4] = h->sblk_arena;
  } else {
    bufs[0] = h->p_recv[SIDE_F]; bufs[1] = h->w_recv[SIDE_F]; bufs[2] = h->p_recv[SIDE_G]; bufs[3] = h->w_recv[SIDE_G]; bufs[4] = h->sblk_arena;
  }
  bufs[5] = h->p2p_flags;
}

int resnmtf_p2p_export(resnmtf_handle* h, void* handles, size_t capacity, size_t* bytes) {
  if (!h || !bytes) return RESNMTF_ERR_INVALID;
  if (!h->opt.slice_p2p) return h->fail(RESNMTF_ERR_STATE, "not a slice_p2p handle");
  *bytes = 6 * sizeof(hipIpcMemHandle_t);
  if (!handles || capacity < *bytes) return h->fail(RESNMTF_ERR_INVALID, "handle buffer too small");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  void* bufs[6];
  p2p_buffers(h, bufs);
  auto* out = static_cast<hipIpcMemHandle_t*>(handles);
  std::memset(out, 0, *bytes);
  for (int b = 0; b < 6; ++b)
    if (bufs[b]) HIP_TRY(h, hipIpcGetMemHandle(&out[b], bufs[b]));
  return RESNMTF_OK;
}

int resnmtf_p2p_import(resnmtf_handle* h, int rank, const void* handles, size_t bytes) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (!h->opt.slice_p2p) return h->fail(RESNMTF_ERR_STATE, "not a slice_p2p handle");
  if (rank < 0 || rank >= h->V) return h->fail(RESNMTF_ERR_INVALID, "rank out of range");
  resnmtf_handle::Peer& pc = h->peers[(size_t)rank];
  if (pc.imported) return h->fail(RESNMTF_ERR_STATE, "rank already imported");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  void* ptr[6];
  void* own[6];
  p2p_buffers(h, own);
  if (rank == h->opt.slice_index) {
    for (int b = 0; b < 6; ++b) ptr[b] = own[b];
  } else {
    if (!handles || bytes < 6 * sizeof(hipIpcMemHandle_t)) return h->fail(RESNMTF_ERR_INVALID, "handle buffer too small");
    const auto* in = static_cast<const hipIpcMemHandle_t*>(handles);
    for (int b = 0; b < 6; ++b) {
      ptr[b] = nullptr;
      if (!own[b]) continue;              // (every rank has the same layout: a buffer this rank lacks, the peer lacks too)
      HIP_TRY(h, hipIpcOpenMemHandle(&ptr[b], in[b], hipIpcMemLazyEnablePeerAccess));
      pc.opened[b] = ptr[b];
    }
  }
  if (h->block_p2p) {
    pc.arena[SIDE_F] = static_cast<char*>(ptr[0]); pc.arena[SIDE_G] = static_cast<char*>(ptr[2]);
  } else {
    pc.p_recv[SIDE_F] = static_cast<char*>(ptr[0]); pc.w_recv[SIDE_F] = static_cast<float*>(ptr[1]); pc.p_recv[SIDE_G] = static_cast<char*>(ptr[2]);
    pc.w_recv[SIDE_G] = static_cast<float*>(ptr[3]);
  }
  pc.sblk = static_cast<double*>(ptr[4]); pc.flags = static_cast<unsigned int*>(ptr[5]);
  pc.imported = true;
  h->p2p_ready = true;
  for (const auto& q : h->peers) h->p2p_ready = h->p2p_ready && q.imported;
  h->prepared = false;
  return RESNMTF_OK;
}

// Every rank calls this at about the same time, after all imports and a host barrier, before resnmtf_prepare.  Host-side
// deadlines everywhere: a node on which peer stores, remote atomics or the stream wait do not work is reported, not hung on.
int resnmtf_p2p_selftest(resnmtf_handle* h, int timeout_ms) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (!h->opt.slice_p2p) return h->fail(RESNMTF_ERR_STATE, "not a slice_p2p handle");
  if (!h->p2p_ready) return h->fail(RESNMTF_ERR_STATE, "slice_p2p: import every rank's buffers first (resnmtf_p2p_import)");
  if (h->p2p_prepared) return h->fail(RESNMTF_ERR_STATE, "resnmtf_p2p_selftest precedes resnmtf_prepare (it writes into the receive buffers)");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  const int V = h->V, r = h->opt.slice_index, kProbeFlag = 8, kWords = 256;
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms > 0 ? timeout_ms : 10000);
  // where rank `from` writes on rank `on` (a place the run prologue overwrites): block form -- the head of view `from`'s U
  // rows in the F arena; sliced form -- the head of chunk `from` of the U receive buffer
  auto region = [&](char* f_arena, char* u_recv, int from) -> unsigned int* {
    if (h->block_p2p) return reinterpret_cast<unsigned int*>(f_arena + (static_cast<const char*>(h->views[(size_t)from].side[SIDE_F].xblk) - static_cast<const char*>(h->arena[SIDE_F])));
    return reinterpret_cast<unsigned int*>(u_recv + (size_t)from * h->p_chunk[SIDE_F]);
  };
  // host-side waits, all under the one deadline
  auto poll_flag = [&](int flag, unsigned int want, const char* what) -> int {
    unsigned int seen = 0;
    for (;;) {
      HIP_TRY(h, hipMemcpy(&seen, h->p2p_flags + flag, sizeof(seen), hipMemcpyDeviceToHost));
      if (seen >= want) return RESNMTF_OK;
      if (std::chrono::steady_clock::now() > deadline) {
        char msg[200];
        std::snprintf(msg, sizeof(msg), "slice_p2p self-test: %u of %u %s within the deadline (peer atomics do not reach this rank)", seen, want, what);
        return h->fail(RESNMTF_ERR_HIP, msg);
      }
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
  };
  auto drain_stream = [&](int flag) -> int {
    for (;;) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) return RESNMTF_OK;
      if (q != hipErrorNotReady) return h->fail_hip("hipStreamQuery", q);
      if (std::chrono::steady_clock::now() > deadline) {
        // last resort so that the handle can still be destroyed: satisfy the wait from the host (the error is what the caller acts on)
        const unsigned int all = 0x7FFFFFFFu;
        (void)hipMemcpy(h->p2p_flags + flag, &all, sizeof(all), hipMemcpyHostToDevice);
        return h->fail(RESNMTF_ERR_HIP, "slice_p2p self-test: hipStreamWaitValue32 does not see the arrival counter");
      }
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
  };
  int* bad = nullptr; int* bad_dev = nullptr;
  HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&bad), sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
  *bad = 0;
  struct Guard { int* p; ~Guard() { if (p) (void)hipHostFree(p); } } guard{bad};
  HIP_TRY(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&bad_dev), bad, 0));
  const int kAckFlag = 9;
  // Two rounds with different words.  Each: store to every peer + one arrival on every rank's counter; the host sees the V
  // arrivals; the stream wait of the phases + a kernel that reads what arrived (as in a sweep -- the second round reads lines
  // the first left in this device's caches); an acknowledgement round so that nobody overwrites what a peer has not read yet.
  for (int round = 0; round < 2; ++round) {
    const unsigned int step = 2u * h->probe_epoch + (unsigned)round;
    auto tag_of = [&](int rank) { return 0xA5000000u | ((unsigned)rank << 16) | ((step & 0xFFu) << 8); };
    P2pProbeArgs a{};
    a.tag = tag_of(r);
    for (int c = 0; c < V; ++c)
      if (c != r) a.dst[a.n_dst++] = region(h->peers[(size_t)c].arena[SIDE_F], h->peers[(size_t)c].p_recv[SIDE_F], r);
    if (a.n_dst) hipLaunchKernelGGL(p2p_probe_kernel, dim3(1), dim3(kWords), 0, h->stream, a);
    p2p_signal(h, kProbeFlag);
    HIP_TRY(h, hipGetLastError());
    const unsigned int want = (unsigned)V * (step + 1);
    if (int rc = poll_flag(kProbeFlag, want, "arrivals")) return rc;
    HIP_TRY(h, hipStreamWaitValue32(h->stream, h->p2p_flags + kProbeFlag, want, hipStreamWaitValueGte, 0xFFFFFFFFu));
    P2pCheckArgs ck{};
    for (int c = 0; c < V; ++c)
      if (c != r) { ck.src[ck.n_src] = region(static_cast<char*>(h->arena[SIDE_F]), h->p_recv[SIDE_F], c); ck.tag[ck.n_src++] = tag_of(c); }
    ck.bad = bad_dev;
    if (ck.n_src) hipLaunchKernelGGL(p2p_check_kernel, dim3(1), dim3(kWords), 0, h->stream, ck);
    HIP_TRY(h, hipGetLastError());
    if (int rc = drain_stream(kProbeFlag)) return rc;
    if (*bad) {
      char msg[200];
      std::snprintf(msg, sizeof(msg), "slice_p2p self-test: %d words read by a kernel after the stream wait are not what the peers stored (round %d%s)",
                    *bad, round, round ? ": stale cache lines" : "");
      return h->fail(RESNMTF_ERR_HIP, msg);
    }
    p2p_signal(h, kAckFlag);                                   // "I have read round `round`"
    HIP_TRY(h, hipGetLastError());
    if (int rc = poll_flag(kAckFlag, want, "acknowledgements")) return rc;
  }
  h->probe_epoch += 1;
  for (int c = 0; c < V; ++c)
    if (c != r) HIP_TRY(h, hipMemset(region(static_cast<char*>(h->arena[SIDE_F]), h->p_recv[SIDE_F], c), 0, kWords * sizeof(unsigned int)));
  return RESNMTF_OK;
}

int resnmtf_kernel_timings(resnmtf_handle* h, double* ms_total, long long* launches, int reset) {
  if (!h || !ms_total || !launches) return RESNMTF_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = flush_timing(h)) return rc;
  for (int i = 0; i < RESNMTF_TIMED_KINDS; ++i) { ms_total[i] = h->ktime_ms[i]; launches[i] = h->klaunch[i]; }
  if (reset)
    for (int i = 0; i < RESNMTF_TIMED_KINDS; ++i) { h->ktime_ms[i] = 0.0; h->klaunch[i] = 0; }
  return RESNMTF_OK;
}

int resnmtf_view_errors(resnmtf_handle* h, int v, int first, int count, double* out) {
  if (int rc = check_view(h, v)) return rc;
  if (!out || first < 0 || count < 0) return h->fail(RESNMTF_ERR_INVALID, "bad error range");
  if (first + count > h->err_cap) return h->fail(RESNMTF_ERR_INVALID, "range beyond the reserved error buffer");
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  // (sweep t of the latest run / of the phases since resnmtf_prepare sits in row (base + t) mod capacity)
  std::vector<double> buf((size_t)h->err_cap * h->V);
  if (count > 0)
    HIP_TRY(h, hipMemcpy(buf.data(), h->err, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int t = 0; t < count; ++t) out[t] = buf[(size_t)((h->sweep_base + first + t) % h->err_cap) * h->V + v];
  return RESNMTF_OK;
}

int resnmtf_synchronize(resnmtf_handle* h) {
  if (!h) return RESNMTF_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = sync_both(h)) return rc;
  if (h->fuse_err && *h->fuse_err == 2) {
    *h->fuse_err = 0;
    return h->fail(RESNMTF_ERR_HIP, "a peer-store wait gave up (p2p_wait_kernel: the arrivals of an exchange never came): results are invalid");
  }
  if (h->fuse_err && *h->fuse_err) {
    *h->fuse_err = 0;
    return h->fail(RESNMTF_ERR_HIP, "a fused pass launch gave up waiting for its update blocks (pass_fused_kernel): results are invalid");
  }
  return RESNMTF_OK;
}

#ifdef RESNMTF_STAMPS
// diagnostic build only: point the stamp buffer at `buf` ([blocks][16] u64) or detach it (NULL)
int resnmtf_debug_set_stamp_buffer(unsigned long long* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf)) == hipSuccess ? 0 : RESNMTF_ERR_HIP;
}
// 1 = only the pass launches stamp, 2 = only the update kernels, 3 = both (they share the columns)
int resnmtf_debug_set_stamp_select(int sel) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_sel), &sel, sizeof(sel)) == hipSuccess ? 0 : RESNMTF_ERR_HIP;
}
#endif

int resnmtf_view_image_info(resnmtf_handle* h, int v, int* uses_2byte, double* rel_error) {
  if (int rc = check_view(h, v)) return rc;
  const ViewState& vs = h->views[v];
  if (uses_2byte) *uses_2byte = vs.half ? (vs.u16 ? 2 : 1) : 0;
  if (rel_error) *rel_error = vs.half_capable ? vs.x_relerr : 0.0;
  return RESNMTF_OK;
}

// the launch plan of view v: what resolve_pass / plan_f_chain decide (tests assert which launch forms they cover)
int resnmtf_view_plan(resnmtf_handle* h, int v, resnmtf_view_plan_info* out) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (!out) return h->fail(RESNMTF_ERR_INVALID, "out is NULL");
  if (out->struct_size != (int)sizeof(resnmtf_view_plan_info)) return h->fail(RESNMTF_ERR_INVALID, "view plan struct_size mismatch");
  if (int rc = check_view(h, v)) return rc;
  const ViewState& vs = h->views[v];
  resnmtf_view_plan_info p;
  std::memset(&p, 0, sizeof(p));
  p.struct_size = (int)sizeof(p);
  p.k = vs.k; p.kp = vs.KP; p.nt = vs.NT;
  p.kk_mode = vs.kk_mode;
  for (int i = 0; i < 2; ++i) {
    const bool xg = i == 0;
    const PassLaunch L = resolve_pass(h, vs, xg);
    p.image = L.image;
    if (L.image >= 2) p.half_unroll = L.unroll;
    p.wide[i] = L.wide; p.xcd_order[i] = L.xcd_order; p.waves[i] = L.waves; p.pingpong[i] = L.pingpong;
    p.unroll[i] = L.image == 0 ? L.unroll : 0;
    const Side &sd = vs.side[i], &red = vs.side[other(i)];      // (i = the side the pass feeds; it reduces over the other)
    p.nsplit[i] = sd.nsplit;
    p.rows[i] = red.len; p.rows_pad[i] = red.pad; p.ntiles[i] = sd.pad / 64;
    if (L.image != 1) { p.rows_per_split[i] = sd.rps; p.short_last[i] = L.short_last; }
    p.tiles_per_wg[i] = L.tiles_per_wg;
    p.aux_splits[i] = L.mode_a ? 0 : sd.nsaux;
    p.sparse_blocks[i] = L.image == 1 ? sd.sp_nblk : 0;
  }
  if (!vs.sparse) {
    p.pitch_pad = vs.side[SIDE_G].ldx != (size_t)vs.n_pad * 64 ? 1 : 0;
    p.lds_pad_kb = h->opt.pass_lds_pad_kb;
  }
  p.prepared = h->prepared ? 1 : 0;
  const FChainPlan fc = h->prepared ? plan_f_chain(h) : FChainPlan{};
  if (fc.hoisted) { p.f_chain_hoisted = 1; p.f_chain_views = fc.width; p.f_chain_one_slab = fc.one_slab; }
  *out = p;
  return RESNMTF_OK;
}

// the update side of view v: the template arguments launch_update hands select_update and the run-time buckets of
// factor_update_body, each read where the launch reads it (couple_bucket, update_threads, the UpdateArgs / KKSArgs that
// build_args filled, Side::rpb / nblk)
int resnmtf_update_plan(resnmtf_handle* h, int v, resnmtf_update_plan_info* out) {
  if (!h) return RESNMTF_ERR_INVALID;
  if (!out) return h->fail(RESNMTF_ERR_INVALID, "out is NULL");
  if (out->struct_size != (int)sizeof(resnmtf_update_plan_info)) return h->fail(RESNMTF_ERR_INVALID, "update plan struct_size mismatch");
  if (int rc = check_view(h, v)) return rc;
  const ViewState& vs = h->views[v];
  resnmtf_update_plan_info p;
  std::memset(&p, 0, sizeof(p));
  p.struct_size = (int)sizeof(p);
  p.prepared = h->prepared ? 1 : 0;
  p.k = vs.k; p.kp = vs.KP;
  p.threads = update_threads(vs.KP);
  p.rows_per_group = p.threads / vs.KP;
  p.emit = vs.kk_mode == 0 ? 1 : 0;
  p.mm64 = update_mm64(vs.KP) ? 1 : 0;
  p.packk = update_packk(vs.KP, p.emit != 0) ? 1 : 0;
  const bool hoist = h->prepared && plan_f_chain(h).hoisted;
  for (int s = 0; s < 2; ++s) {
    const Side& sd = vs.side[s];
    const UpdateArgs& u = sd.arg;
    // (before the first prepare the argument block is empty: the slabs are then those fill_update will copy from the side)
    p.nsplit[s] = h->prepared ? u.nsplit : (sd.xsum ? 1 : sd.nsplit);
    p.split_bucket[s] = update_split_bucket(p.nsplit[s]);
    p.rows_per_block[s] = sd.rpb; p.nblk[s] = sd.nblk;
    p.last_block_rows[s] = sd.len - (sd.nblk - 1) * sd.rpb;
    if (!h->prepared) continue;
    p.restricted[s] = u.restricted; p.n_couple[s] = u.n_couple;
    p.couple_bucket[s] = couple_bucket(u);
    for (int c = 0; c < u.n_couple; ++c) ++(u.couple[c].map ? p.n_index_maps : p.n_identity_maps)[s];
    p.sigma_is_zero[s] = u.sigma == 0.0 ? 1 : 0;
    p.route[s] = (s == SIDE_F && hoist) ? 2 : (can_fuse_update(h, vs, s) ? 1 : 0);
  }
  if (h->prepared) { p.s_restricted = vs.argKS.restricted; p.s_n_couple = vs.argKS.n_couple; }
  *out = p;
  return RESNMTF_OK;
}

int resnmtf_pass_timings(resnmtf_handle* h, resnmtf_pass_timing* out, int reset) {
  if (!h || !out) return RESNMTF_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->opt.device_id));
  if (int rc = flush_timing(h)) return rc;
  *out = h->timing;
  // algorithmic bytes / flops of ONE launch of the first owned view's passes
  for (const auto& v : h->views) {
    if (!v.owned) continue;
    const double n = v.n, m = v.m, k = v.k;
    const PassLaunch L = resolve_pass(h, v, true);
    const double sx = L.image >= 2 ? 2.0 : 4.0;    // bytes per element of X as stored
    // (a launch that carries the update of its B operand -- pass_fused_kernel -- also moves that update's algorithmic bytes:
    //  product rows 4 len k once, the fp64 factor 8 len k in and out, its f32 copy 4 len k out)
    out->xg_bytes = sx * n * m + 4.0 * (n + m) * k + (can_fuse_update(h, v, 1) ? 24.0 * m * k : 0.0);
    out->xtf_bytes = sx * n * m + 4.0 * (n + m) * k + (can_fuse_update(h, v, 0) && h->all_owned && h->chain_views[SIDE_F] == 0 ? 24.0 * n * k : 0.0);
    out->xg_flops = 2.0 * n * m * k;
    out->xtf_flops = 2.0 * n * m * k;
    if (L.image == 1) {      // values + indices + pointers + gathered factor rows (f32, KP wide) + slabs written
      const double z = (double)v.nnz, kp = v.KP;
      out->xg_bytes = 8.0 * z + 8.0 * (n + 1) + 4.0 * kp * z + 4.0 * kp * n * v.side[SIDE_F].nsplit;
      out->xtf_bytes = 8.0 * z + 8.0 * (m + 1) + 4.0 * kp * z + 4.0 * kp * m * v.side[SIDE_G].nsplit;
      out->xg_flops = out->xtf_flops = 2.0 * z * k;
    }
    break;
  }
  if (reset) h->timing = resnmtf_pass_timing{};
  return RESNMTF_OK;
}

}  // extern "C"
