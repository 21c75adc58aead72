/*
 * resnmtf_hip.h -- C-ABI of the MI355X-native ResNMTF multiplicative-update inner loop.
 *
 * The reference (eso28599/resnmtf, pure R) has NO native boundary (NAMESPACE:1-4 has no
 * useDynLib, there is no src/).  The seam is cut around the body of the iteration loop of
 * res_nmtf_inner (R/main.r:48-109): {update_matrices x T, calculate_error x T} plus the
 * post-loop normalisation_check (R/utils.r:176-195) and the binary cluster matrices of
 * obtain_biclusters (R/obtain_bicl.r:162-180).  Each entry point below cites the reference
 * code it replaces.  See INTEGRATION.md for the R-side .Call() binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every call returns 0 on success, non-zero on error; resnmtf_last_error() gives the text.
 *     No exception crosses the ABI.
 *   - all host matrices are fp64 COLUMN-MAJOR (R's native layout): element (i, j) of an
 *     r x c matrix is at [i + j * r].  Vectors are plain fp64 arrays.
 *   - the caller owns every host buffer; the library copies during the call.  The handle owns
 *     all device memory.  A handle is not re-entrant; calls block unless stated otherwise.
 *   - views, rows and columns are 0-based.
 *   - there is NO CPU fallback: every compute entry point fails with RESNMTF_ERR_NO_DEVICE when
 *     no gfx950 device is usable.
 */
#ifndef RESNMTF_HIP_H
#define RESNMTF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RESNMTF_ABI_VERSION 2   /* 2: options gained wait_mode and the sliced-chain fields, bf16_split = 1 is refused, new phases / selectors / entry points */
#define RESNMTF_MAX_K 64

enum {
  RESNMTF_OK = 0,
  RESNMTF_ERR_INVALID = 1,   /* bad argument / call order */
  RESNMTF_ERR_NO_DEVICE = 2, /* no usable HIP device */
  RESNMTF_ERR_HIP = 3,       /* a HIP runtime call failed */
  RESNMTF_ERR_ALLOC = 4,
  RESNMTF_ERR_STATE = 5      /* handle not prepared / view not owned */
};

/* factor selectors for resnmtf_factor_device_ptr */
enum { RESNMTF_FACTOR_F = 0, RESNMTF_FACTOR_G = 1, RESNMTF_FACTOR_S = 2,
       RESNMTF_FACTOR_FBLOCK = 3, /* replicate_f: the F update's inputs [U (X.G, one f32 slab) | Ma_F | Md_F | lambda], contiguous */
       RESNMTF_FACTOR_FBLOCK_ALL = 4 /* replicate_f: the blocks of ALL views, contiguous in view order (v is ignored beyond its
                                        range check); equal-shaped views have equal block sizes, so one in-place all-gather
                                        over ranks that own one view each refreshes every block */,
       RESNMTF_FACTOR_GBLOCK = 5, /* replicate_gs: the G update's inputs [T (Xt.F, one f32 slab) | Ma_G | Md_G | mu] of view v */
       RESNMTF_FACTOR_GBLOCK_ALL = 6, /* ... of all views, contiguous in view order */
       RESNMTF_FACTOR_SBLOCK = 7, /* replicate_gs: the S update's inputs of view v (fp64: old S | F^T X G | (F^T F S)(G^T G) |
                                     G^T G | F^T F | colSums(G) | colSums(F) | ||X||^2) */
       RESNMTF_FACTOR_SBLOCK_ALL = 8 /* ... of all views, contiguous in view order (equal k: equal blocks).  With equal-shaped
                                        views the S block of a view sits at the end of its F block instead (the address
                                        RESNMTF_FACTOR_SBLOCK returns lies inside RESNMTF_FACTOR_FBLOCK's range): gathering
                                        the F blocks after RESNMTF_PHASE_XG moves both, and this selector is refused */,
       /* slice_chains: the buffers of the four all-to-all exchanges of a sweep (fp32; V equal chunks each, chunk c = what
        * rank c receives / what came from rank c; `v` is ignored beyond its range check) */
       RESNMTF_FACTOR_U_SEND = 9,    /* own view's U = X.G' folded, cut into V row slices          [V][rows_per_slice][KP] */
       RESNMTF_FACTOR_U_RECV = 10,   /* rows of MY slice of every view's U                          (same shape) */
       RESNMTF_FACTOR_FNEW_SEND = 11,/* new F rows of my slice of every view (compact f32)         [V][rows_per_slice][KP] */
       RESNMTF_FACTOR_FNEW_RECV = 12,/* the own view's new F, all rows, as the V slice holders sent them */
       RESNMTF_FACTOR_T_SEND = 13,   /* own view's T = Xt.F' in V column slices, each followed by Ma_G | Md_G (fp64) */
       RESNMTF_FACTOR_T_RECV = 14,
       RESNMTF_FACTOR_GNEW_SEND = 15,
       RESNMTF_FACTOR_GNEW_RECV = 16,
       RESNMTF_FACTOR_F_SLICE = 17,  /* the rows of MY slice of view v's fp64 F (a range inside RESNMTF_FACTOR_F): during a sliced
                                        run these are the only rows of any view's F this rank keeps current -- collect the
                                        slices (all-gather) before reading a whole factor */
       RESNMTF_FACTOR_G_SLICE = 18 };

/* phases of one view's update inside a sweep (R/update_steps.r:282-314) */
enum {
  RESNMTF_PHASE_F = 0, /* update_f (R/update_steps.r:141-165) incl. star_prod_relevant (R/utils.r:63-78) */
  RESNMTF_PHASE_G = 1, /* Xt.F pass, update_g (R/update_steps.r:180-207), X.G' pass; update_s (220-240),
                          update_lm x2 (249-251, 312-313) and calculate_error (R/utils.r:157-166) ride in
                          the X.G' launch */
  RESNMTF_PHASE_S = 2, /* no work: marks the point after which the view's new S may be exchanged */
  RESNMTF_PHASE_F_ALL = 3 /* update_f of EVERY view whose F inputs this handle holds (owned views and, with replicate_f, the
                             others), in view order; `v` only has to be a valid view.  F_w' does not read G or S of this
                             sweep, so hoisting the F updates of a sweep in front of its PHASE_G calls changes nothing.
                             One launch (f_chain_kernel) when k <= 16, the views have equal row counts, share their rows in
                             the same order and at most four of them are owned; one launch per view otherwise.  resnmtf_run
                             hoists the F updates of a sweep the same way when that launch applies */,
  RESNMTF_PHASE_LOCAL_SWEEP = 4 /* RESNMTF_PHASE_F_ALL followed by RESNMTF_PHASE_G of every owned view: everything a rank
                             does between two exchanges of the F blocks when no G or S crosses ranks, in one call */,
  /* replicate_gs (view argument = any owned view for the _ALL phases):
   *   sweep = F_ALL, XTF(own), [all-gather G blocks], G_ALL, XG(own), [all-gather S blocks], S_ALL, [all-gather F blocks] */
  RESNMTF_PHASE_XTF = 5   /* Xt.F pass of owned view v + its k x k job (F'^T F', Ma_G, Md_G) + fold of T into the G block */,
  RESNMTF_PHASE_G_ALL = 6 /* update_g of EVERY view, in view order (R/update_steps.r:180-207, :295-303) from the G blocks; one launch when
                             the views have equal column counts and share their columns in the same order (f_chain_kernel's G form at
                             k <= 16, wide_chain_kernel above), one per view otherwise */,
  RESNMTF_PHASE_XG = 7    /* X.G' pass of owned view v + first half of its k x k job (inputs of the S rule -> S block) +
                             fold of U into the F block */,
  RESNMTF_PHASE_S_ALL = 8 /* update_s, update_lm, error and the F coefficients of EVERY view (s_chain_kernel) */,
  /* slice_chains (view argument = the owned view):
   *   sweep = SLICE_F, [all-to-all: new F rows -> owners], SLICE_XTF, [all-to-all: T slices + G coefficients],
   *           SLICE_G, [all-to-all: new G rows -> owners], SLICE_XG, [all-gather S blocks] S_ALL  ||  [all-to-all: U slices] */
  RESNMTF_PHASE_SLICE_F = 9   /* update_f of EVERY view on MY row slice, in view order (R/update_steps.r:141-165, :282-287) */,
  RESNMTF_PHASE_SLICE_XTF = 10 /* received F rows -> operand copies; Xt.F pass + k x k job of the owned view; T cut into slices */,
  RESNMTF_PHASE_SLICE_G = 11  /* update_g of EVERY view on MY column slice (R/update_steps.r:180-207, :295-303) */,
  RESNMTF_PHASE_SLICE_XG = 12 /* received G rows -> operand copies; X.G' pass + first half of the k x k job (S block); U cut into slices */
};

typedef struct resnmtf_handle resnmtf_handle;

typedef struct resnmtf_options {
  int struct_size;        /* = sizeof(resnmtf_options); set by resnmtf_default_options */
  int device_id;          /* HIP device ordinal; one process per GPU (default 0) */
  void* stream;           /* hipStream_t to enqueue on; NULL = library-owned stream */
  int use_graph;          /* 1 (default): the sweeps of a run are replayed from captured hipGraphs (one graph of the exact
                             length for short fixed runs, else batches of check_every and a power-of-two ladder for the rest) */
  int check_every;        /* convergence mode: sweeps enqueued per host-side check (default 32; launches after the stop
                             test fired return at once) */
  int target_workgroups;  /* workgroup slots a streaming pass is sized for (>= 64, smaller values are refused); 0 = default: CUs x resident workgroups per CU
                             (two at k <= 16, one above) */
  int time_kernels;       /* 1: bracket every streaming-pass launch with HIP events (eager mode) */
  /* tuning overrides of the streaming-pass geometry (0 = automatic), see DESIGN.md section 5 */
  int pass_waves;         /* waves per workgroup: 4, 8 or 16 (0 = auto) */
  int pass_splits_xg;     /* row splits of the X.G pass: 0 (default) = the launch model's choice, else 1 ... 16 (refused beyond) */
  int pass_splits_xtf;    /* row splits of the Xt.F pass: likewise */
  int pass_lds_pad_kb;    /* extra dynamic LDS per workgroup (caps workgroups per CU) */
  int update_blocks;      /* workgroups per factor-update launch; 0 = default: ~160 (512 above 256 MB of X) in hand-off
                             mode A, one round of resident workgroups (CUs x 1 at k > 32, x 2 at k = 32) in mode B */
  int no_pitch_pad;       /* 1: do not pad row pitches that are multiples of 4 KiB (A/B testing) */
  int kk_mode;            /* where the k x k products come from: 0 auto, 1 = A (fp64 partials of the update
                             kernels, job in workgroup 0 of the pass launch), 2 = B (MFMA aux tiles, job in
                             the last-arriving aux workgroup); DESIGN.md section 4 */
  int bf16_split;         /* MFMA form of the two big contractions for k > 16 (k <= 16 always uses the f32 MFMA):
                             0 (default) both operands as THREE bf16 pieces (each rounded to nearest even; X split in
                               registers, the factor's pieces written K-packed by the update kernels), six
                               v_mfma_f32_16x16x32_bf16 per product group in WIDE workgroups (8 or 4 tiles share one
                               LDS copy of the factor block) -- dropped terms <= 2^-26: f32-grade (F / G 2e-7 ... 7e-6
                               from the fp64 reference, the f32 MFMA 1e-7 ... 6e-6);
                             1 refused (RESNMTF_ERR_INVALID): the former two-piece form is retired -- callers that asked
                               for its speed / precision trade must choose 0 or 2 knowingly;
                             2 plain v_mfma_f32_16x16x4_f32, one tile per workgroup */
  int replicate_f;        /* view-sharded use (phase API): 1 = every rank keeps, for EVERY view, the inputs of its F
                             update (X.G folded into one f32 slab, the two k x k coefficient matrices, lambda) in one
                             contiguous exchange block (RESNMTF_FACTOR_FBLOCK) and may run RESNMTF_PHASE_F on views it does
                             not own: the host moves the blocks once per sweep (one all-gather, or one broadcast per
                             view) after the owners' PHASE_G and every rank
                             computes the phi-coupled F chain locally -- identical kernels on identical bytes,
                             so bitwise the same F everywhere -- instead of waiting for N serial F broadcasts */
  int no_f_chain;         /* 1: RESNMTF_PHASE_F_ALL always issues one launch per view (A/B testing) */
  int x_half;             /* (3: as 2, but per view only when the image's relative quantisation error || X~ - X || / || X ||,
                             measured at upload, is at most 3e-5 -- F / G move by 0.2 ... 2 x that error; else the f32 images.)
                             (2: as 1 with UNIFORM 16-bit integers -- one power-of-two step per view -- widened exactly to f32 and
                             multiplied on the f32 MFMA: F / G within 1e-6 ... 3e-5, inside the bar on every problem tried.)
                             1: k <= 16 -- the two passes stream a K-packed fp16 image of X (per-view power-of-two scale, 11-bit
                             mantissa) instead of the f32 one: half the bytes; the factor operand stays f32-grade (two fp16
                             pieces, 22 bits), f32 accumulate.  F / G then sit within ~2e-5 of the fp64 reference instead of
                             ~1e-6 (bar 1e-4); DESIGN.md section 3 */
  int half_unroll;        /* 2-byte passes: wave-steps (16 rows each) per trip: 2, 3, 4 or 6 (0 = default: 4 for fp16, 2 for integers) */
  int replicate_gs;       /* view-sharded use, with replicate_f: 1 = the G and S chains are replicated too.  Every rank keeps,
                             for EVERY view, the inputs of its G update (Xt.F folded into one f32 slab, Ma_G, Md_G, mu:
                             RESNMTF_FACTOR_GBLOCK) and of its S update (old S, F^T X G, (F^T F S)(G^T G), the two Gram
                             matrices, column sums, ||X||^2: RESNMTF_FACTOR_SBLOCK), runs RESNMTF_PHASE_G_ALL /
                             RESNMTF_PHASE_S_ALL for all views itself and only streams its own X (RESNMTF_PHASE_XTF /
                             RESNMTF_PHASE_XG): two all-gathers per sweep (T blocks; U blocks with the S blocks inside --
                             three, S blocks on their own, when the views' F blocks differ in size) instead of
                             2 V ordered broadcasts, and the two streaming passes of all ranks run at the same time
                             (psi / xi coupling; R/update_steps.r:195-204, :231-237).  Needs equal k in all views. */
  int wait_mode;          /* how a fixed-iteration resnmtf_run waits for the device: 0 (default) polls the sweep counter the last
                             k x k job mirrors into pinned host memory -- the call returns when the counter arrives, which can be
                             up to ~100 us BEFORE the stream has drained (every other entry point synchronises first), and the
                             calling thread spins (with pauses) meanwhile, at most 20 ms without progress before it falls back to
                             a stream synchronisation; 1 = hipStreamSynchronize (blocks, ~10-15 us later per call) */
  int slice_chains;       /* view-sharded use, with replicate_f and replicate_gs: 1 = ROW-SLICED chains.  star_prod_relevant is
                             row-local by name (R/utils.r:67-73), so instead of every rank walking the whole F (G) chain of all
                             V views, rank r walks it for the 1 / V of the shared rows (columns) it is assigned
                             (RESNMTF_PHASE_SLICE_F / _G): one view's worth of element-wise work per rank.  The rows travel by
                             all-to-all (the RESNMTF_FACTOR_*_SEND / _RECV buffers), the S chain stays replicated (k x k).  Needs
                             one owned view per handle (view index = slice_index), slice_count = number of views <= 8, equal
                             shapes and k, every coupled pair sharing ALL rows / columns in the same order (identity maps);
                             hand-off mode B is used at every k.  Otherwise fall back to replicate_gs. */
  int slice_index;        /* which slice this handle walks (= the rank) */
  int slice_count;        /* number of slices (= ranks = views) */
  int slice_p2p;          /* with slice_chains (opt-in): the four exchanges of a sweep as PEER STORES + stream-ordered flags instead
                             of collectives -- the chain kernels and slice_pack_kernel store their output straight into the
                             receiving rank's buffers (mapped through hipIpc: xGMI peer access across GPUs), a one-wave kernel then
                             adds one arrival to every rank's counter of that exchange, and the consuming phase begins with a
                             hipStreamWaitValue32 for the V arrivals of its sweep: no collective launch, no host in the loop, no
                             device-side spin.  Set-up: resnmtf_p2p_export on every rank, the handles exchanged by the host
                             (any channel), resnmtf_p2p_import for every rank (the own one included), a host barrier, then ONE
                             resnmtf_prepare.  Receive buffers are single: the order of the sweep itself keeps a writer one
                             exchange behind its reader.  Tested with 2-4 processes on one GPU (IPC on one
                             device); not yet run across GPUs: resnmtf_p2p_selftest tells whether a node can run it.
                             WITHOUT slice_chains (block form; needs replicate_f, one owned view = slice_index, slice_count =
                             number of views <= 8): the exchange blocks of the replicated layouts are stored into every peer's
                             arena instead of all-gathered -- replicate_gs: behind RESNMTF_PHASE_XTF (T rows + G coefficients) and
                             RESNMTF_PHASE_XG (U rows + S block), G_ALL / S_ALL wait for the V arrivals of their sweep;
                             replicate_f alone: the sweep is RESNMTF_PHASE_LOCAL_SWEEP, which waits for the V blocks of the
                             previous sweep, acknowledges them after its F chain and stores its own block after V
                             acknowledgements.  The first blocks (after resnmtf_prepare) travel by the caller's collective,
                             followed by a synchronise + barrier before the first phase.
                             2: as 1 with every wait as a one-wave KERNEL instead of hipStreamWaitValue32 (device counters number
                             the waits, the spin sleeps between polls and is bounded: resnmtf_synchronize reports a wait that gave
                             up) -- kernel nodes only, so whole sweeps can be captured in a graph and replayed by the caller.
                             Bitwise the same results (tested in all three layouts); measured no faster than 1 (the sweep is not
                             bound by the host's launches): opt-in */
  int xcd_order;          /* 1 (opt-in): the main workgroups of the k > 16 passes renumbered so that every XCD works through a
                             contiguous range of the split-major list -- a row split's B block is then fetched into one or two
                             L2s instead of all eight (c5 Xt.F: 154 MB of 1.78 GB per launch).  Measured (tools/round3/xcd_ab.sh):
                             c4 view +0.7 %, c5 X.G pass +1 %, c5 Xt.F pass -5 % (430 against 409 us) -- the passes are not
                             bound by those bytes, and concentrating an XCD on one row range costs more than the re-reads: off */
  int fuse_updates;       /* 0 (default): every factor update is a launch of its own.  1 / 2 (opt-in, k <= 16, hand-off mode A, f32
                             images): an UNCOUPLED update_f / update_g (R/update_steps.r:152-155 / :190-193) runs in the first
                             workgroups of the Xt.F / X.G' launch that consumes it, the other workgroups wait for it on an arrival
                             flag (1: with the first trip of X rows requested before the wait, 2: without).  Bitwise the same
                             results (tested), one launch per update less -- but MEASURED SLOWER on MI355X (c2: 52 - 62 us per
                             sweep against 43): publishing a row block to the other XCDs takes an agent-scope release (an L2
                             write-back), 0.3 - 0.5 us per workgroup and serial within an XCD, so the flag rises 4 - 7 us after the
                             last block is done (profiles/r03_stamps_fused_c2_*.txt) */
} resnmtf_options;

typedef struct resnmtf_pass_timing {
  double xg_ms_total;     /* summed duration of the X.G streaming-pass launches */
  double xtf_ms_total;    /* summed duration of the Xt.F streaming-pass launches */
  long long xg_launches;
  long long xtf_launches;
  double xg_bytes;        /* algorithmic bytes of ONE X.G launch   */
  double xtf_bytes;       /* algorithmic bytes of ONE Xt.F launch */
  double xg_flops;        /* algorithmic flops of ONE X.G launch  */
  double xtf_flops;
} resnmtf_pass_timing;

int resnmtf_abi_version(void);
/* number of visible HIP devices (0 when none; never fails) */
int resnmtf_device_count(void);
void resnmtf_default_options(resnmtf_options* opts);
/* text of the last error on this handle (or of the last failed resnmtf_create when h == NULL) */
const char* resnmtf_last_error(const resnmtf_handle* h);

/*
 * Create a handle for n_views views; view v is n_rows[v] x n_cols[v] with k[v] biclusters
 * (2 <= k <= RESNMTF_MAX_K).  owned[v] != 0 marks the views whose data matrix lives on THIS
 * process' GPU (owned == NULL: all).  Non-owned views only have factor mirrors (F, G, S) that
 * the host refreshes through resnmtf_factor_device_ptr + its own exchange (RCCL broadcast).
 * Replaces: the R lists built by res_nmtf_inner, R/main.r:38-48.
 */
int resnmtf_create(int n_views, const int* n_rows, const int* n_cols, const int* k,
                   const int* owned, const resnmtf_options* opts, resnmtf_handle** out);
int resnmtf_destroy(resnmtf_handle* h);

/*
 * Sparse data views.  As resnmtf_create, with nnz_capacity[v] per view: < 0 = a dense view (exactly as resnmtf_create
 * makes it), >= 0 = a SPARSE view that holds at most that many stored entries.  A sparse view allocates no dense image of
 * X (8 n m bytes), only a CSC copy (int64 column pointers, int32 row indices, fp32 values) for the Xt.F' pass and a CSR
 * copy (likewise) for the X.G pass: 16 bytes per entry + 8 (n + m).  Its passes are sparse-times-dense kernels that write
 * the same partial slabs as the dense passes, so the rest of the sweep (updates, k x k chains, error, stop test) is the
 * dense path's; hand-off mode A at every k; x_half, fuse_updates and the view-sharded layouts (replicate_f / replicate_gs /
 * slice_chains / slice_p2p: refused) never apply.  resnmtf_get_view, resnmtf_copy_view, resnmtf_shuffle_view and
 * resnmtf_subsample_view refuse a sparse view (RESNMTF_ERR_INVALID) instead of densifying it; a sparse view is shuffled
 * by resnmtf_shuffle_view_sparse, copied by resnmtf_copy_view_sparse and sub-sampled by resnmtf_subsample_view_sparse (it
 * stays sparse), and read back by resnmtf_get_view_csc.
 * resnmtf_bisil refuses one too (RESNMTF_ERR_STATE: it reads the fp32 images); resnmtf_bisil_sparse scores it from the
 * CSC / CSR copies.
 * Replaces: as resnmtf_create (R/main.r:38-48) for views that R holds as Matrix::dgCMatrix (R/utils.r:416-419 densifies
 * them with as.matrix; the result is defined as the factorisation of that dense matrix).
 */
int resnmtf_create_sparse(int n_views, const int* n_rows, const int* n_cols, const int* k, const int* owned,
                          const long long* nnz_capacity, const resnmtf_options* opts, resnmtf_handle** out);
/*
 * Upload the data of a sparse owned view as 0-based CSC: col_ptr [m + 1] (int64), row_idx / values [col_ptr[m]] -- the
 * @p / @i / @x slots of a dgCMatrix.  Checked on the host before any device work (RESNMTF_ERR_INVALID, text in
 * resnmtf_last_error): col_ptr[0] = 0 and monotone, col_ptr[m] <= the view's capacity, row indices in range and strictly
 * increasing within a column, finite non-negative values.  pre_processed = 0: check_inputs on the device --
 * matrix_normalisation (x / colSums(x), R/utils.r:86-88), fp64, before the f32 copies; an all-zero column is refused (the
 * reference yields a NaN column) and so is a negative entry (make_non_neg's per-column shift, R/utils.r:20-27, would turn
 * every implicit zero positive: shift on the host and upload dense).  pre_processed = 1: values taken as given (the
 * sub-samples of stability selection).  Then data_norms (R/main.r:48) as resnmtf_set_view.  The CSR copy is built here
 * (entries of a row in ascending column order), and the work split of the two passes is planned from the row / column
 * lengths.
 */
int resnmtf_set_view_csc(resnmtf_handle* h, int v, const long long* col_ptr, const int* row_idx, const double* values,
                         int pre_processed);
/* Storage of view v: *is_sparse (0 / 1), *nnz = stored entries of the last upload (0 for dense views), *nnz_capacity (-1 for
 * dense views).  Any pointer may be NULL. */
int resnmtf_view_storage(resnmtf_handle* h, int v, int* is_sparse, long long* nnz, long long* nnz_capacity);
/*
 * shuffle_view (R/obtain_bicl.r:11-22) of a SPARSE view into a sparse view of another (or the same) handle, on the device:
 * exactly resnmtf_shuffle_view's draw of the densified source -- the same Feistel permutation of the n m positions for the
 * same `seed` -- built from the stored entries alone.  The shuffle holds the source's nnz stored entries (explicit zeros
 * included) and no dense image is allocated at any point.  normalise != 0: matrix_normalisation (R/utils.r:86-88) of the
 * shuffle, fp64, as apply_resnmtf applies it to shuffled data (R/obtain_bicl.r:35 -> R/utils.r:416,422; the values are
 * non-negative, so make_non_neg shifts nothing); normalise == 0: the values as they are.  Then data_norms, the CSR copy and
 * the work split of the passes as resnmtf_set_view_csc: the view is bit for bit the one resnmtf_set_view_csc makes of the
 * same shuffle built on the host from the source's stored fp32 values, with pre_processed = !normalise.  The redraw
 * condition of the reference (:14-18; a line is empty when it holds no stored entry > 0) is reported by
 * resnmtf_view_empty_lines, as after resnmtf_shuffle_view; the caller redraws with another seed.
 * Refused: a dense dst or src view, a shape mismatch, another device, src's nnz above dst's capacity (RESNMTF_ERR_INVALID);
 * a view that is not owned, a source that has not been uploaded (RESNMTF_ERR_STATE).
 */
int resnmtf_shuffle_view_sparse(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, unsigned long long seed,
                                int normalise);
/*
 * Sub-samples and copies of sparse views on the device (DESIGN.md section 10 "Device copies and sub-samples").
 *
 * resnmtf_subsample_count_sparse: the number of stored entries (stored zeros included) of X[rows, cols] of sparse view
 * v_src -- what the nnz_capacity of a destination for resnmtf_subsample_view_sparse must be at least.  rows holds n_rows
 * and cols n_cols 0-based indices, in any order; nothing is built and the view is not changed.
 * Replaces: the size of data[[i]][row_samples[[i]], col_samples[[i]]] (R/stability_analysis.r:124, :184, :232, :238),
 * which R's Matrix package finds while it builds the sub-matrix.
 *
 * resnmtf_subsample_view_sparse: dst's sparse view v = X[rows, cols] of src's sparse view v_src, as a sparse view.  rows
 * holds dst view v's n entries, cols its m entries, as in resnmtf_subsample_view, in any order (R's sample is unsorted:
 * destination row i is source row rows[i]).  The values are carried over as stored, fp32, NOT re-normalised;
 * stored zeros stay stored.  The view is bit for bit -- pointers, indices, both value arrays, data_norms, the work split of
 * the passes -- the one resnmtf_set_view_csc(pre_processed = 1) makes of the same sub-sample built on the host from
 * resnmtf_get_view_csc of the source.  The rows and columns without a stored entry > 0 (the trimming condition,
 * R/stability_analysis.r:165-190, :233-240) are reported by resnmtf_view_empty_lines, as after resnmtf_subsample_view.
 * Replaces: data[[i]][row_samples[[i]], col_samples[[i]]] (R/stability_analysis.r:124, :184, :232, :238).
 *
 * resnmtf_copy_view_sparse: dst's sparse view v = src's sparse view v_src, device to device, as resnmtf_copy_view does for
 * dense views (the k sweep, R/main.r:279-290, factorises the same data for every k); k may differ between the handles --
 * the work split of the passes is planned again for dst's k.  Bit for bit resnmtf_set_view_csc(pre_processed = 1) of the
 * source's read-back on dst, with the source's data_norms.
 *
 * Refused on the host before any launch, the destination left as it was (RESNMTF_ERR_INVALID): NULL arguments, a dense
 * source or destination (resnmtf_subsample_view / resnmtf_copy_view take those), handles on different devices, for the
 * copy views that differ in shape, an index out of range, an index that occurs twice in rows or in cols (the reference
 * samples without replacement); a view that is not owned or a source that has not been uploaded (RESNMTF_ERR_STATE).
 * A destination whose nnz_capacity is below the stored entries of the sub-sample (known after the counting pass, which
 * writes nothing of dst) or of the source is refused too (RESNMTF_ERR_INVALID; the text names both numbers).
 */
int resnmtf_subsample_count_sparse(resnmtf_handle* src, int v_src, int n_rows, const int* rows, int n_cols, const int* cols,
                                   long long* nnz);
int resnmtf_subsample_view_sparse(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, const int* rows,
                                  const int* cols);
int resnmtf_copy_view_sparse(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src);
/*
 * The device CSC copy of a sparse view back on the host: col_ptr [m + 1], row_idx / values [nnz] (nnz from
 * resnmtf_view_storage; values at fp32 precision) -- the @p / @i / @x slots of the dgCMatrix that R/utils.r:416-419 would
 * densify.  Any pointer may be NULL.  A dense view is refused (RESNMTF_ERR_INVALID: resnmtf_get_view reads it); nothing is
 * densified.
 */
int resnmtf_get_view_csc(resnmtf_handle* h, int v, long long* col_ptr, int* row_idx, double* values);

/*
 * Upload the data matrix of an owned view: x is n x m fp64 column-major, ALREADY non-negative
 * and column-L1-normalised (what check_inputs produces, R/utils.r:416,422).  Also computes
 * data_norms[v] = ||X||_F^2 (R/main.r:48) on the device.
 */
int resnmtf_set_view(resnmtf_handle* h, int v, const double* x);

/*
 * Upload a RAW data matrix and pre-process it on the device, fused into the upload pass:
 * make_non_neg_inner (per COLUMN shift by |min(0, min(column))|, R/utils.r:20-27) followed by
 * matrix_normalisation (divide by colSums, R/utils.r:86-88) -- what check_inputs does at
 * R/utils.r:416,422 -- then data_norms as above.  *was_negative (may be NULL) is set to 1 when an
 * entry was negative, the condition of the reference's warning (R/utils.r:23-25).  A zero column
 * yields NaN, as in the reference.
 */
int resnmtf_set_view_raw(resnmtf_handle* h, int v, const double* x_raw, int* was_negative);

/*
 * The same two uploads for a dense matrix that is ALREADY in device memory, in any of four floating types and with
 * any (non-negative) strides, without a host copy and without an fp64 staging buffer: element (r, c) of the n x m view
 * is x[r * row_stride + c * col_stride], strides in ELEMENTS (column-major: 1, n; row-major: m, 1; transposed views and
 * slices likewise; x points at element (0, 0)).  raw == 0 takes the values as resnmtf_set_view does (already non-negative
 * and column-normalised, R/utils.r:416,422); raw != 0 runs make_non_neg_inner and matrix_normalisation on the device as
 * resnmtf_set_view_raw does (R/utils.r:20-27,86-88) and reports *was_negative (may be NULL); data_norms (R/main.r:48)
 * either way.  Widening to fp64 is exact for all four types and every sum keeps the order of the host route, so the
 * images, data_norms and *was_negative are BIT FOR BIT those of resnmtf_set_view / resnmtf_set_view_raw of the same
 * values widened on the host.  A zero column yields NaN as there; resnmtf_view_empty_lines reports zero, as after a
 * host upload.
 *   stream  the hipStream_t on which the producer of x was enqueued (NULL: the null stream).  The library records an
 *           event there and makes its own stream wait for it.  The call returns when the images are built
 *           (as resnmtf_set_view does), so x may be freed on return.
 * Refused before any device work (RESNMTF_ERR_INVALID / _STATE, text in resnmtf_last_error): x == NULL, an unknown
 * dtype, a negative stride, a pointer that is not device memory of the handle's device, a view the handle does not
 * own, a sparse view (resnmtf_set_view_csc).
 */
enum { RESNMTF_DTYPE_F64 = 0, RESNMTF_DTYPE_F32 = 1, RESNMTF_DTYPE_F16 = 2, RESNMTF_DTYPE_BF16 = 3 };
int resnmtf_set_view_device(resnmtf_handle* h, int v, const void* x, int dtype, long long row_stride, long long col_stride,
                            int raw, int* was_negative, void* stream);

/*
 * Upload the data of a sparse owned view from arrays that are ALREADY in device memory -- what torch's sparse_csc,
 * sparse_csr and (coalesced) sparse_coo tensors hold -- without a host copy: nothing runs per entry on the host.
 *   layout      RESNMTF_SPARSE_CSC: ptr_or_rows = the m + 1 column pointers, idx_or_cols = the row index of every entry;
 *               RESNMTF_SPARSE_CSR: the n + 1 row pointers and the column indices;
 *               RESNMTF_SPARSE_COO: nnz row indices and nnz column indices.
 *   index_type  RESNMTF_INDEX_I32 / _I64, one type for both index arrays; dtype: RESNMTF_DTYPE_* of values [nnz].
 *               Every array is contiguous and 0-based.
 *   stream      as for resnmtf_set_view_device: an event recorded there, the handle's stream waits for it, and the call
 *               returns when the view is built, so the arrays may be freed on return.
 * The entries may come in ANY order (within a column, within a row, arbitrary for COO).  Stored positions must be
 * distinct: a position stored twice is refused (the caller coalesces; nothing is summed).  Explicit zeros stay stored.
 * pre_processed as for resnmtf_set_view_csc: 0 = matrix_normalisation (R/utils.r:86-88) on the device, a column without
 * an entry > 0 refused; 1 = the values as they are.
 * The view is BIT FOR BIT the one resnmtf_set_view_csc makes of the canonical CSC (columns ascending, rows ascending
 * within a column, explicit zeros kept) of the same (row, column, value widened to fp64) set: both pointer and index
 * arrays, both value arrays, data_norms, the work split of the passes, resnmtf_view_empty_lines reporting zero.
 * Widening is exact, the positions are distinct (so their sorted order is unique), and normalisation, the CSR values,
 * data_norms and the plan are the host route's own code.  A CSC input whose rows already ascend strictly within every
 * column skips the first of the two sorts.  nnz = 0 is accepted with pre_processed = 1.
 * Transient device memory: 40 bytes per entry (the sparse shuffle's build) + m bytes + 16.
 * Refused before any device work (RESNMTF_ERR_INVALID / _STATE, text in resnmtf_last_error): a NULL array (values /
 * idx_or_cols, and COO's rows, may be NULL only when nnz = 0), an unknown layout, index type or dtype, nnz < 0 or above
 * the view's capacity, a dense view, a view the handle does not own, an array that is not device memory of the handle's
 * device.  Refused by the device checks (RESNMTF_ERR_INVALID; the text names the condition and the lowest offending
 * line, entry or position): pointers that do not start at 0, are not monotone or do not end at nnz; an index out of
 * range; a non-finite or negative value; a position stored twice; with pre_processed = 0 an all-zero column (nnz = 0:
 * every column).  Every refusal leaves the view exactly as it was.
 * Replaces: as resnmtf_set_view_csc (R/utils.r:416-419 for a Matrix::dgCMatrix), for data produced on the device.
 */
enum { RESNMTF_SPARSE_CSC = 0, RESNMTF_SPARSE_CSR = 1, RESNMTF_SPARSE_COO = 2 };
enum { RESNMTF_INDEX_I32 = 0, RESNMTF_INDEX_I64 = 1 };
int resnmtf_set_view_sparse_device(resnmtf_handle* h, int v, int layout, const void* ptr_or_rows, const void* idx_or_cols,
                                   int index_type, const void* values, int dtype, long long nnz, int pre_processed,
                                   void* stream);

/*
 * View data without a host round trip (the callers of the loop repeat it 36-66 times per apply_resnmtf):
 *   resnmtf_copy_view     device copy of an uploaded view of another handle on the same GPU (same n x m) --
 *                         the k sweep (R/main.r:279-290) factorises ONE data set for every k;
 *   resnmtf_shuffle_view  shuffle_view (R/obtain_bicl.r:11-22): all n m entries of the source view permuted
 *                         pseudo-randomly on the device (Feistel network with cycle walking, `seed`), then
 *                         -- normalise != 0 -- non-negativity shift + column normalisation as apply_resnmtf
 *                         applies to the shuffled data (R/obtain_bicl.r:35 -> R/utils.r:416,422).  R's own
 *                         sample() stream cannot be reproduced.  The reference redraws while a row or a column
 *                         of the shuffled matrix sums to zero (:14-18): resnmtf_view_empty_lines reports that
 *                         condition for the draw just made, the caller redraws with another seed;
 *   resnmtf_subsample_view  the sub-sample X[rows, cols] of stability_repeat (R/stability_analysis.r:230-249; dst's
 *                         shape = the index counts; 0-based indices into the source view), NOT re-normalised,
 *                         exactly as the reference factorises it; all-zero rows / columns
 *                         of the sub-sample (the reference drops them, R/stability_analysis.r:165-190, :233-240)
 *                         are reported by resnmtf_view_empty_lines, masks included;
 *   resnmtf_get_view      the device copy back as fp64 column-major (fp32 precision), e.g. for a host-side
 *                         SVD or for tests.
 */
int resnmtf_copy_view(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src);
int resnmtf_shuffle_view(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, unsigned long long seed,
                         int normalise);
int resnmtf_subsample_view(resnmtf_handle* dst, int v, resnmtf_handle* src, int v_src, const int* rows, const int* cols);
/* Rows / columns of view v's data that summed to exactly zero when it was last drawn on the device
 * (resnmtf_shuffle_view, resnmtf_subsample_view; before any shift / normalisation): counts, and -- if not NULL --
 * 0 / 1 masks of length n and m.  Zero after a host upload (the host has the data). */
int resnmtf_view_empty_lines(resnmtf_handle* h, int v, int* n_empty_rows, int* n_empty_cols, unsigned char* row_mask,
                             unsigned char* col_mask);
int resnmtf_get_view(resnmtf_handle* h, int v, double* x);

/*
 * The data a handle holds, written to caller-owned DEVICE memory without a host round trip: the pre-processed matrix the
 * library factorises (R/utils.r:416,422), a shuffle drawn on the device (R/obtain_bicl.r:11-22) or a stability
 * sub-sample gathered there (R/stability_analysis.r:230-249).
 *
 * resnmtf_get_view_device: element (r, c) of dense view v is written to out[r * row_stride + c * col_stride], strides in
 * ELEMENTS (column-major: 1, n; row-major: m, 1; slices and transposes of a contiguous buffer likewise).  dtype is
 * RESNMTF_DTYPE_F64 or _F32.  The values are BIT FOR BIT those of resnmtf_get_view: the stored f32 image, widened exactly
 * or kept.  One kernel reads the tile-major image through an LDS tile and writes with neighbouring lanes along the
 * smaller of the two strides; no atomics, no transient device memory.
 *   stream  as for resnmtf_finalise_device: the library's writes are ordered after the work already enqueued there and
 *           before any work enqueued there after the call returns.
 * Refused before any device work, out untouched (RESNMTF_ERR_INVALID unless noted): out == NULL or not device memory of
 * the handle's device; RESNMTF_DTYPE_F16 / _BF16 (narrowing is not a copy) or an unknown dtype; a stride <= 0 along an
 * extent > 1; strides under which two elements would share an address (with a <= b the two strides and e the extent
 * along a: a (e - 1) < b is required); a sparse view (resnmtf_get_view_sparse_device); a view that is not owned or has
 * no data (RESNMTF_ERR_STATE).
 *
 * resnmtf_get_view_sparse_device: the mirror of resnmtf_set_view_sparse_device.
 *   layout      RESNMTF_SPARSE_CSC: ptr_or_rows receives the m + 1 column pointers, idx_or_cols the row index and values
 *               the value of every stored entry -- the CSC copy: columns ascending, rows ascending within a column,
 *               explicit zeros kept; BIT FOR BIT resnmtf_get_view_csc;
 *               RESNMTF_SPARSE_CSR: the n + 1 row pointers, column indices and values of the CSR copy, columns ascending
 *               within a row: what the canonical CSR of that CSC holds;
 *               RESNMTF_SPARSE_COO: nnz row and nnz column indices in the CSR copy's order (row-major sorted, what
 *               torch calls coalesced); the row pointers are expanded to a row index per entry on the device.
 *   index_type  RESNMTF_INDEX_I32 / _I64 for both index arrays (the stored pointers are int64 and the stored indices
 *               int32: one of them is converted on the device); I32 is refused when nnz exceeds 2^31 - 1.
 *   dtype       RESNMTF_DTYPE_F64 or _F32 of values.
 * Sizes from resnmtf_view_storage.  Any of the three arrays may be NULL and is then skipped; nnz = 0 writes the pointers
 * only.  stream as above.  No transient device memory.
 * Refused before any device work (RESNMTF_ERR_INVALID unless noted): a dense view; an unknown layout, index type or
 * dtype; a 16-bit dtype; a non-NULL array that is not device memory of the handle's device; a view that is not owned or
 * has no data (RESNMTF_ERR_STATE).
 * Replaces: the dgCMatrix slots R/utils.r:416-419 would densify, as resnmtf_get_view_csc, for a caller on the device.
 */
int resnmtf_get_view_device(resnmtf_handle* h, int v, void* out, int dtype, long long row_stride, long long col_stride,
                            void* stream);
int resnmtf_get_view_sparse_device(resnmtf_handle* h, int v, int layout, void* ptr_or_rows, void* idx_or_cols,
                                   int index_type, void* values, int dtype, void* stream);

/*
 * Initial factors of view v (owned or mirror): F n x k, S k x k, G m x k, column-major.
 * lambda / mu may be NULL: they are then colSums(F) / colSums(G), the reference's
 * explicit-init branch (R/update_steps.r:49-56).
 */
int resnmtf_set_factors(resnmtf_handle* h, int v, const double* F, const double* S,
                        const double* G, const double* lambda, const double* mu);

/*
 * The same for initial factors that are ALREADY in device memory (R/update_steps.r:41-56), in any of the four floating
 * types and with any (non-negative) strides, without a host copy: nothing runs per element on the host.  A matrix is
 * (ptr, dtype, row_stride, col_stride): ptr points at element (0, 0), element (r, c) is ptr[r * row_stride +
 * c * col_stride], strides in ELEMENTS (column-major n x k: 1, n; row-major: k, 1; transposed views and slices likewise);
 * one dtype per matrix.  F n x k, S k x k, G m x k; lambda / mu k x 1 (col_stride is not read), or NULL: they are then
 * colSums(F) / colSums(G) (R/update_steps.r:55-56), summed on the device per column in ascending row order from 0.0, as
 * resnmtf_set_factors sums them.  Widening to fp64 is exact for all four types, so the view's whole factor state is BIT
 * FOR BIT what resnmtf_set_factors leaves when given the same values widened on the host (the operand images are built
 * by the same code).  Values are not validated (NaN, Inf and negative entries pass, as there).  Works for an owned or
 * a mirror view, dense or sparse.  The sources must not overlap the handle's own buffers.
 *   stream  the hipStream_t on which the producer of the matrices was enqueued (NULL: the null stream).  The library
 *           records an event there and makes its own stream wait for it.  The call returns when the state is built, so
 *           the sources may be freed on return.
 * Refused before any device work (RESNMTF_ERR_INVALID / _STATE, text in resnmtf_last_error), the view's factors and
 * whether it has any left as they were: a NULL handle, a bad view, F / S / G NULL or with a NULL ptr, lambda / mu with
 * a NULL ptr, an unknown dtype, a negative stride, a pointer that is not device memory of the handle's device, lambda
 * or mu for a view the handle does not own (RESNMTF_ERR_STATE).
 * No transient device memory.
 */
typedef struct {
  const void* ptr;                     /* element (0, 0) */
  int dtype;                           /* RESNMTF_DTYPE_* */
  long long row_stride, col_stride;    /* in ELEMENTS, >= 0 */
} resnmtf_device_matrix;
int resnmtf_set_factors_device(resnmtf_handle* h, int v, const resnmtf_device_matrix* F, const resnmtf_device_matrix* S,
                               const resnmtf_device_matrix* G, const resnmtf_device_matrix* lambda,
                               const resnmtf_device_matrix* mu, void* stream);

/*
 * Initial factors of an owned view from its data: init_mats_inner (R/update_steps.r:78-125) --
 * F0 = |U[, 1:k]|, G0 = |V[, 1:k]| of the SVD of X, S0 = |diag(d)[1:k, 1:k]| + |N(0, sigma I)| noise,
 * S0 columns scaled by colSums(F0) * colSums(G0), F0 and G0 column-L1-normalised, lambda / mu their
 * column sums.  The reference calls a full svd(); here the k leading triplets come from a randomized
 * subspace iteration (n_power >= 1 iterations, 0 = default 3; sketch width 16 ceil((k + 8) / 16) <= 64)
 * whose big products are the streaming-pass kernels, and the noise from a std::mt19937_64 seeded with
 * `seed` (R's RNG / MASS::mvrnorm are not reproducible outside R): statistically, not bitwise,
 * equivalent; singular vectors of (near-)equal singular values are determined up to rotation in
 * either implementation.  Views whose short side is smaller than the sketch take an exact route instead
 * (Gram matrix of the short side, Jacobi).  sigma = 0.05 is the reference's default.  singular_values (k, may be NULL)
 * receives d[1:k].  Requires resnmtf_set_view / resnmtf_set_view_raw; replaces resnmtf_set_factors.
 */
int resnmtf_init_svd(resnmtf_handle* h, int v, unsigned long long seed, double sigma, int n_power,
                     double* singular_values);

/*
 * resnmtf_init_svd with a read-back of the signed basis it takes |.| of (resnmtf_init_svd is this call without the
 * read-back: the same arithmetic, the same factors).  Column-major fp64: U receives the k leading left vectors (n x k),
 * V the right ones (m x k), d ALL singular values the route computed, in descending order (room for 64), and *n_d their
 * count: min(L, min(n, m)), L the sketch width.  U = Q Ut and V = X^T Q Ut / d are formed in fp64 from the sketch's
 * last orthonormal basis Q; X^T Q is the last streaming pass (f32).  A triplet past the numerical rank of X (the rank
 * cut of the sketch's CholeskyQR2, or an exactly zero eigenvalue) has d = 0 and zero vectors here; the factors then
 * hold the constant unit vector in its place (svd() returns some unit vector there).
 * U, V, d, n_d must not be NULL (RESNMTF_ERR_INVALID); singular_values may be.
 */
int resnmtf_init_svd_basis(resnmtf_handle* h, int v, unsigned long long seed, double sigma, int n_power,
                           double* singular_values, double* U, double* V, double* d, int* n_d);

/*
 * Restriction matrices, n_views x n_views column-major, ALREADY symmetrised with zero diagonal
 * (the output of init_rest_mats, R/update_steps.r:12-24).  NULL = all zero.
 */
int resnmtf_set_restrictions(resnmtf_handle* h, const double* phi, const double* xi,
                             const double* psi);

/*
 * Shared rows (columns) between views v and w, as index pairs: row idx_v[t] of view v carries
 * the same NAME as row idx_w[t] of view w.  This is the integer form of
 * row_indices[[v]][[as.character(w)]] (R/utils.r:560-601) after match() against the row names.
 * count = -1 encodes the reference's NA ("no shared names"): star_prod_relevant then skips
 * the numerator term for w (R/utils.r:70) while update_f still adds phi[w,v]*F to the
 * denominator (R/update_steps.r:158).  Pairs that were never set default to NA.
 * Must be called for (v, w) and for (w, v) separately, as the reference keeps one map per
 * ordered pair.
 */
int resnmtf_set_shared_rows(resnmtf_handle* h, int v, int w, int count, const int* idx_v,
                            const int* idx_w);
int resnmtf_set_shared_cols(resnmtf_handle* h, int v, int w, int count, const int* idx_v,
                            const int* idx_w);

/*
 * Run the loop of res_nmtf_inner (R/main.r:50-109) on a handle that owns every view.
 *   n_iters  > 0 : fixed number of sweeps (R/main.r:83-108).
 *   n_iters == 0 : convergence mode, stop after the first sweep t with
 *                  |mean_err_t - mean_err_{t-1}| <= tol, mean_err_0 = 0 (R/main.r:53-81;
 *                  the reference uses tol = 1e-6), or after max_iters sweeps (a guard the
 *                  reference lacks; max_iters <= 0 means err_capacity).
 * all_err[t] receives mean over views of ||X - F S G^T||_F^2 / ||X||_F^2 after sweep t
 * (All_Error, R/main.r:78,104); err_capacity is the length of all_err.  iters_done receives
 * the number of sweeps executed.  May be called repeatedly; state carries over.
 * Fixed-iteration runs wait on a host-mapped sweep counter (options.wait_mode = 0): the call may return while the stream is
 * still draining the last launch's workgroups, and the calling thread polls meanwhile -- see resnmtf_options.wait_mode;
 * every other entry point, resnmtf_synchronize included, waits for the stream.
 */
int resnmtf_run(resnmtf_handle* h, int n_iters, double tol, int max_iters, double* all_err,
                int err_capacity, int* iters_done);

/* Raw (un-normalised) state, so that a caller can resume exactly.  Any pointer may be NULL. */
int resnmtf_get_factors(resnmtf_handle* h, int v, double* F, double* S, double* G,
                        double* lambda, double* mu);
/*
 * The same raw state (R/update_steps.r:41-56: what the explicit-init branch takes), bitwise, written to caller-owned
 * DEVICE buffers on the handle's device: fp64 column-major F n x k, S k x k, G m x k, lambda and mu of length k; any may
 * be NULL.  `stream` as for resnmtf_finalise_device: the library's writes are ordered after the work already enqueued
 * there and before any work enqueued there after the call returns.  Refused before any device work: a pointer that is
 * not device memory of the handle's device (RESNMTF_ERR_INVALID), lambda / mu of a view the handle does not own
 * (RESNMTF_ERR_STATE).  No transient device memory.
 */
int resnmtf_get_factors_device(resnmtf_handle* h, int v, double* F, double* S, double* G,
                               double* lambda, double* mu, void* stream);

/*
 * normalisation_check (R/utils.r:176-195) followed by the binary cluster matrices of
 * obtain_biclusters with remove_spurious = FALSE (R/obtain_bicl.r:162-180):
 * row_clusters = 1[F > 1/n][, relations], col_clusters = 1[G > 1/m], relations[j] =
 * which.max(S[, j]).  Does not modify the handle's state.  Any output pointer may be NULL.
 */
int resnmtf_finalise(resnmtf_handle* h, int v, double* F, double* S, double* G,
                     double* row_clusters, double* col_clusters);
/*
 * The same (same kernels, same bits: R/utils.r:176-195, R/obtain_bicl.r:162-180), written to caller-owned DEVICE
 * buffers on the handle's device: fp64 column-major, n x k, k x k, m x k, n x k, m x k; any may be NULL.  `stream` is
 * the hipStream_t the caller works on (NULL: the null stream): the library's writes are ordered after the work already
 * enqueued there and before any work enqueued there after the call returns.  A pointer that is not device memory of the
 * handle's device is refused before any device work.
 */
int resnmtf_finalise_device(resnmtf_handle* h, int v, double* F, double* S, double* G,
                            double* row_clusters, double* col_clusters, void* stream);

/*
 * Stability selection (stability_check, R/stability_analysis.r:302-338) scores every sub-sample's factorisation
 * against the original result.  Two entries replace the scoring step of stability_repeat (:268-276):
 *
 *   resnmtf_set_reference_clusters  the original result's binary clusters for view v: n_rows[v] x k and n_cols[v] x k,
 *                         column-major 0 / 1 fp64 as resnmtf_finalise emits them (results$row_clusters[[v]],
 *                         results$col_clusters[[v]]); k may differ from the handle's own k[v] (e.g. a data-only
 *                         handle that the sub-samples are gathered from).  Kept on the device as bytes; a second call
 *                         replaces them.  Entries other than 0 / 1 are refused (RESNMTF_ERR_INVALID).
 *   resnmtf_relevance     relevance_results(row_c, col_c, true_r, true_c) (R/stability_analysis.r:45-67, with
 *                         jaccard_main :16-33 and cart_prod / jaccard_func R/utils.r:117-145) for view v of h:
 *                         row_c / col_c = the clusters resnmtf_finalise would return for h's current F, S, G
 *                         (computed on the device, same kernels and comparisons; nothing is copied back and h's state
 *                         is not modified), true_r = ref_row[rows, ], true_c = ref_col[cols, ] = the clusters set on
 *                         ref's view v_ref gathered by h's n_rows[v] / n_cols[v] 0-based indices.  relevance receives
 *                         k doubles: max over h's clusters i of the Jaccard index of the pair sets R_i x C_i and
 *                         TR_j x TC_j, for every reference cluster j; 0 for every j when exactly one of row_c / true_r
 *                         has no non-empty column, 1 when neither has.  Counted in integers, one fp64 division per
 *                         pair: bitwise equal to an fp64 restatement.  Refused before any launch: NULL pointers, a bad
 *                         view or handle, handles on different devices (RESNMTF_ERR_INVALID), no reference clusters
 *                         on ref's view or no factors on h's (RESNMTF_ERR_STATE), the reference's k differing from
 *                         h's k[v], indices out of range (RESNMTF_ERR_INVALID).
 */
int resnmtf_set_reference_clusters(resnmtf_handle* h, int v, int k, const double* row_clusters, const double* col_clusters);
int resnmtf_relevance(resnmtf_handle* h, int v, resnmtf_handle* ref, int v_ref, const int* rows, const int* cols,
                      double* relevance);

/*
 * resnmtf_set_reference_clusters for cluster matrices that are ALREADY in device memory (results$row_clusters[[v]] /
 * results$col_clusters[[v]] of R/stability_analysis.r:268-276, as resnmtf_finalise_device leaves them): n x k and m x k,
 * 0 / 1, each a resnmtf_device_matrix as resnmtf_set_factors_device takes one -- any of the four floating types, any
 * non-negative strides.  They are read in place after an event recorded on `stream` and may be freed on return.  Every
 * entry is checked on the device: anything other than 0 or 1 is refused (RESNMTF_ERR_INVALID; NaN included; -0.0 counts
 * as 0, as on the host route), with the message of row_clusters if that matrix has a bad entry, otherwise that of
 * col_clusters.  The entries are packed into the same row-major byte block resnmtf_set_reference_clusters uploads, so
 * resnmtf_relevance and resnmtf_relevance_masked return the same bits as after the host route.  Also refused, before any
 * device work: NULL pointers, k outside [1, 64], an unknown dtype, a negative stride, a pointer that is not device
 * memory of the handle's device.  EVERY refusal leaves the view's previous reference clusters exactly as they were (the
 * block is built in a fresh allocation and swapped in only on success).  Transient device memory: 8 bytes.
 */
int resnmtf_set_reference_clusters_device(resnmtf_handle* h, int v, int k, const resnmtf_device_matrix* row_clusters,
                                          const resnmtf_device_matrix* col_clusters, void* stream);

/*
 * Relevance after a spurious-bicluster removal (a stability repeat of res_nmtf_inner(sub_sample, spurious = TRUE),
 * R/stability_analysis.r:254-276): resnmtf_relevance with h's clusters cleaned first as obtain_biclusters does
 * (R/obtain_bicl.r:176-188).  flags: k[v] bytes indexed by F column (nonzero = the removal rule flagged that column's
 * score); cluster column j of both row_c and col_c is zeroed when flags[relations[j]] is set, relations[j] =
 * which.max(S[, j]) computed on the device as resnmtf_finalise computes it.  Same counts, same epilogue: bitwise equal to
 * the fp64 restatement on the cleaned clusters (a mask that empties every cluster included).  Refusals as for
 * resnmtf_relevance, and flags NULL (RESNMTF_ERR_INVALID).
 */
int resnmtf_relevance_masked(resnmtf_handle* h, int v, resnmtf_handle* ref, int v_ref, const int* rows, const int* cols,
                             const unsigned char* flags, double* relevance);

/*
 * Spurious-bicluster scoring (check_biclusters / get_thresholds, R/obtain_bicl.r:55-133): jsd_calc (R/utils.r:95-106)
 * for a list of column pairs, replacing the R loops
 *     scores <- c(scores, jsd_calc(x1, x2))                        (calculate_f_shuffle_jsd, :55-68)
 *     scores[i, k] <- mean(apply(x_noise, 2, function(y) jsd_calc(x, y)))   (check_biclusters, :125-128)
 * cols: n_cols columns of length n, fp64 column-major (an R matrix, e.g. cbind(F_i, f_1[[i]], ..., f_R[[i]]));
 * pairs: n_pairs (x1, x2) 0-based column indices, interleaved; out[p] = jsd_calc(cols[, x1] , cols[, x2]):
 * philentropy::JSD(unit = "log2", est.prob = "empirical") of stats::density(c, from = 0, to = max(x1, x2)) of both
 * sides, n = 512, bw.nrd0 bandwidths, R <= 4.3's density coordinates (old.coords = TRUE), zero beyond max(c).  fp64
 * throughout; bitwise reproducible, and a pair's value depends on its two columns only (not on the other pairs, their
 * order or n_cols).  A density that sums to zero gives NaN, as in R.  No handle: the call selects device_id, uploads,
 * computes and returns (blocking); resnmtf_last_error(NULL) describes a failure.  Refused before any launch
 * (RESNMTF_ERR_INVALID): n < 2, n_cols outside [1, 65535], n_pairs < 0, NULL pointers, a non-finite entry of cols, a
 * pair index outside [0, n_cols), n * n_cols > 2^31; n_pairs = 0 returns at once.  DESIGN.md section 11.
 */
int resnmtf_jsd_pairs(int device_id, int n, int n_cols, const double* cols, int n_pairs, const int* pairs, double* out);

/*
 * resnmtf_jsd_pairs (the same body, kernels, refusals and out, bit for bit) that also hands back what its stages made,
 * for tests of each stage against a reference; every one of the three may be NULL (all NULL = resnmtf_jsd_pairs):
 *   sorted  [n_cols][n]          every column ascending, -0 stored as +0: the buffer the statistics and pair kernels
 *                                read (the last merge destination);
 *   stats   [n_cols][2]          per column bw.nrd0 and the maximum;
 *   dens    [n_pairs][2][512]    per pair, side 0 (x1) then side 1 (x2): stats::density on seq(0, M, length = 512) after
 *                                the values beyond max(c) are zeroed and before the division by the sum.
 * With n_pairs = 0, sorted and stats are still produced when asked for.
 */
int resnmtf_jsd_stages(int device_id, int n, int n_cols, const double* cols, int n_pairs, const int* pairs, double* out,
                       double* sorted, double* stats, double* dens);

/*
 * Spurious-bicluster scores of a factorisation against R shuffled ones, all on the device (check_biclusters with
 * get_thresholds, R/obtain_bicl.r:80-133): view v of h and of each of the R handles in shuffles (same device, same n
 * and k = K, with factors) is normalised as resnmtf_finalise normalises F (F / colSums(F), the same kernels and bits)
 * straight into a device pool cbind(F_v, f_1, ..., f_R) (n x K (R + 1)); resnmtf_jsd_pairs' kernels then score the
 * pairs of calculate_f_shuffle_jsd and check_biclusters over it.  score receives K doubles: score[k] = the mean of
 * jsd_calc(F_v[, k], cbind(f_1..f_R)[, y]) over y = 1 .. R K (R/obtain_bicl.r:125-128), summed in NumPy's pairwise
 * order (np.mean's) so that it equals the host's mean of resnmtf_jsd_pairs' values bitwise.  null_scores receives the
 * K^2 R (R - 1) / 2 null scores in calculate_f_shuffle_jsd's order (j = 1 .. R - 1, k, l = j + 1 .. R, m); their mean
 * and the mode of stats::density stay with the caller.  No factor leaves the device; blocking, on h's stream, after
 * every shuffle handle's stream has drained; deterministic (no atomics in any sum).  Refused before any launch: NULL
 * pointers or handles, a bad view, R < 2, n < 2, a shuffle handle on another device or whose view v differs in n or k,
 * K (R + 1) > 65535, n K (R + 1) > 2^31, more than 2^31 - 1 pairs (RESNMTF_ERR_INVALID), a view without factors
 * (RESNMTF_ERR_STATE).  A non-finite entry of a normalised F is refused after the gather, before the scoring
 * (RESNMTF_ERR_INVALID).  DESIGN.md section 11.
 */
int resnmtf_spurious_scores(resnmtf_handle* h, int v, resnmtf_handle* const* shuffles, int R, double* score,
                            double* null_scores);

/*
 * Bisilhouette (res_nmtf_inner's `bisil`, R/obtain_bicl.r:189-199, and the score the k sweep of apply_resnmtf ranks,
 * R/main.r:291-312 with extract_bisils R/utils.r:203-210): the per-member silhouettes of view v's biclusters that
 *     bisilhouette::bisilhouette(data[[i]], row_clustering[[i]], col_clustering[[i]], method = distance)
 * combines (the combination -- bicluster, view and overall means -- stays on the host, resnmtf_amd/bisil.py).
 * row_clusters / col_clusters: n_rows[v] x k and n_cols[v] x k, column-major 0 / 1 fp64 as resnmtf_finalise emits them;
 * k may differ from the handle's k[v] (e.g. a data-only handle).  Bicluster l = (rows I_l, columns J_l); it is active
 * when both are non-empty.  For a member i of an active I_l: a = mean distance to I_l \ {i}, b = min over the other
 * active l' of the mean distance to I_l' \ {i} (empty sets skipped), both on bicluster l's columns J_l; s = (b - a) /
 * max(a, b), 0 when |I_l| = 1, no l' is left or max(a, b) = 0.  The columns likewise, on the rows I_l.  metric: 0 =
 * euclidean, 1 = manhattan, 2 = cosine (1 - x.y / (|x| |y|); 1 when exactly one norm is 0, 0 when both are).
 * row_sil / col_sil receive n_rows[v] x k and n_cols[v] x k column-major, 0 at non-members and inactive biclusters.
 * The data are the view's fp32 device image (no upload); distances, sums, a, b and s are fp64, every sum in an order
 * fixed by the shapes and clusters (no atomics): bitwise reproducible.  Blocking.  Refused before any launch: NULL
 * pointers, a bad view, k outside [1, 64], entries other than 0 / 1, an unknown metric (RESNMTF_ERR_INVALID); a sparse
 * view (resnmtf_bisil_sparse takes those), a view without data on this handle (RESNMTF_ERR_STATE).  DESIGN.md section 13.
 */
int resnmtf_bisil(resnmtf_handle* h, int v, int k, const double* row_clusters, const double* col_clusters, int metric,
                  double* row_sil, double* col_sil);
/*
 * resnmtf_bisil for a SPARSE view (resnmtf_create_sparse + resnmtf_set_view_csc): the same arguments, outputs,
 * definition and determinism promise, hence the same R lines (bisilhouette::bisilhouette on as.matrix of the view,
 * R/obtain_bicl.r:189-199, R/utils.r:416-419).  No dense image is built: for one side of one bicluster the restricted
 * block G[f][u] = X(U[u], J_l[f]) (features x members of the active biclusters, fp32) is zero-filled and the stored
 * entries of its feature lines are written into it -- columns from the CSC copy for the row side, rows from the CSR copy
 * for the column side -- and the norm, distance and epilogue kernels of resnmtf_bisil run on it.  row_sil / col_sil are
 * bitwise equal to resnmtf_bisil on a dense view that holds the same fp32 values (both uploaded pre-processed); no
 * atomics, two calls give equal bits.  The workspace is sized before it is allocated: the largest block is
 * max_l |J_l| x |U| floats per side, at most one padded dense image; one that exceeds the device's free memory is
 * refused with RESNMTF_ERR_ALLOC and the bytes asked for in resnmtf_last_error.  Refused as resnmtf_bisil refuses, with
 * the same codes; a DENSE view (RESNMTF_ERR_STATE: use resnmtf_bisil), a view without data (RESNMTF_ERR_STATE).
 * DESIGN.md section 13.
 */
int resnmtf_bisil_sparse(resnmtf_handle* h, int v, int k, const double* row_clusters, const double* col_clusters,
                         int metric, double* row_sil, double* col_sil);
/*
 * resnmtf_bisil / resnmtf_bisil_sparse from cluster matrices that are ALREADY in device memory, with the view's score
 * (bisilhouette::bisilhouette's value for the view, R/obtain_bicl.r:189-199) combined on the device too; dense and
 * sparse views alike (the entry dispatches on the view's storage).  row_clusters / col_clusters: n_rows[v] x k and
 * n_cols[v] x k matrices of 0 / 1, each a resnmtf_device_matrix as resnmtf_set_reference_clusters_device takes one -- any
 * of the four floating types, any non-negative strides --, read in place after an event recorded on `stream`; checked on
 * the device (an entry other than 0 or 1, NaN included, is refused with resnmtf_bisil's message, that of row_clusters
 * first; -0.0 is 0).  row_sil / col_sil: DEVICE pointers to n_rows[v] x k and n_cols[v] x k fp64 column-major arrays, or
 * both NULL when only the score is wanted; bit for bit what resnmtf_bisil / resnmtf_bisil_sparse write for the same
 * clusters (the membership words, counts, the union U, rank and every bicluster's member and feature lists are built by
 * kernels in the order the host builds them; the gather / scatter, norm, distance and epilogue kernels are the same).
 * view_score: a HOST pointer to one double, required: per active bicluster l the mean of the row silhouettes over I_l
 * and of the column silhouettes over J_l (members in ascending index order, summed in NumPy's order), sigma_l = half
 * their sum, then the mean of the sigma_l; 0 with fewer than two active biclusters -- resnmtf_amd/bisil.py's view_score,
 * bit for bit.  No active bicluster: zero silhouettes, score 0, RESNMTF_OK.  Blocking.  The host reads back 2 k + 3 ints
 * (the refusal bits, |U| of both sides, the member counts) and the score; nothing of size n or m crosses the bus.
 * Transient device memory beyond resnmtf_bisil's workspace (sized and refused in the same way, RESNMTF_ERR_ALLOC): two
 * u64 arrays and one int array (sparse: two) over n + m points, the int lists and the gathered silhouettes over
 * sum |I_l| + sum |J_l| entries: O(n + m + sum |I_l| + sum |J_l|).  Refused before any device work: NULL descriptors or
 * view_score, k outside [1, 64], an unknown dtype, a negative stride, a matrix or output that is not device memory of
 * the handle's device, an unknown metric (RESNMTF_ERR_INVALID); a view without data, a dense view that holds only a
 * 2-byte image (RESNMTF_ERR_STATE).  A refusal writes neither output.  DESIGN.md section 19.
 */
int resnmtf_bisil_device(resnmtf_handle* h, int v, int k, const resnmtf_device_matrix* row_clusters,
                         const resnmtf_device_matrix* col_clusters, int metric, double* row_sil, double* col_sil,
                         double* view_score, void* stream);

/*
 * Many small factorisations in one launch (the k sweep, the shuffled fits of obtain_shuffled_f, the sub-sample fits of
 * stability_check): res_nmtf_inner (R/main.r:32-140) for every job, one workgroup per job, fp64 throughout.  A job is
 * what res_nmtf_inner receives: pre-processed views, explicit initial factors, symmetrised restrictions and the
 * shared-name index pairs of every view pair (as for resnmtf_set_shared_rows / _cols).  Per job the kernel runs the
 * sweeps of update_matrices (R/update_steps.r:272-319, views in index order), calculate_error as the explicit residual
 * ||X - F S G^T||_F^2 / ||X||_F^2 (R/utils.r:157-166) averaged over the views, the stop rule and normalisation_check
 * (R/utils.r:176-195); outputs are F, S, G (normalised), lambda, mu, All_Error and the sweep count.  The caller derives
 * the binary cluster matrices (R/obtain_bicl.r:162-180) from them.
 *   n_iters > 0: min(n_iters, max_iters) sweeps; n_iters == 0: while |mean_err_t - mean_err_{t-1}| > tol with
 *   mean_err_0 = 0 (R/main.r:53-80), at most max_iters sweeps.
 * Every sum has an order fixed by the job's own shapes and there are no atomics: a job's results are bitwise the same
 * alone, in any batch, at any position and run to run.  Blocking; no handle: the call selects device_id, uploads
 * everything in one buffer, makes one launch per k class present (k <= 8, <= 16, <= 32; each job runs in the kernel
 * instance of its own k) and copies the results back; resnmtf_last_error(NULL) describes a failure.
 * Refused before any device work (RESNMTF_ERR_INVALID): n_jobs < 0, jobs NULL, a struct_size mismatch, max_iters < 1,
 * tol not finite, n_views outside [1, 8], k outside [1, 32] or above a view dimension, n_rows * n_cols above 2^22 for a
 * view, NULL input or output pointers, non-finite inputs, negative restriction entries or a non-zero diagonal, an
 * index pair outside its views, n_iters < 0, err_capacity below the sweeps allowed.  n_jobs = 0 returns at once.
 * DESIGN.md section 12.
 */
#define RESNMTF_GROUP_MAX_VIEWS 8
#define RESNMTF_GROUP_MAX_K 32
#define RESNMTF_GROUP_MAX_VIEW_ENTRIES (1 << 22)
typedef struct resnmtf_group_job {
  int struct_size;                       /* sizeof(resnmtf_group_job) */
  int n_views, k;
  int n_iters;                           /* 0 = run to convergence */
  int n_rows[RESNMTF_GROUP_MAX_VIEWS], n_cols[RESNMTF_GROUP_MAX_VIEWS];
  const double* x[RESNMTF_GROUP_MAX_VIEWS];        /* pre-processed X_v, n x m column-major */
  const double* f0[RESNMTF_GROUP_MAX_VIEWS];       /* initial F_v n x k, S_v k x k, G_v m x k */
  const double* s0[RESNMTF_GROUP_MAX_VIEWS];
  const double* g0[RESNMTF_GROUP_MAX_VIEWS];
  const double* lambda0[RESNMTF_GROUP_MAX_VIEWS];  /* k entries; NULL = colSums(F0) (R/update_steps.r:55) */
  const double* mu0[RESNMTF_GROUP_MAX_VIEWS];      /* k entries; NULL = colSums(G0) */
  const double* phi;                     /* n_views x n_views column-major, symmetrised, zero diagonal; NULL = zeros */
  const double* xi;
  const double* psi;
  /* shared rows / columns of view pair (v, w), v != w: count <= 0 = NA (no shared names), else count positions in
   * view v and in view w (naming.index_pairs) */
  int row_count[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];
  const int* row_idx_v[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];
  const int* row_idx_w[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];
  int col_count[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];
  const int* col_idx_v[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];
  const int* col_idx_w[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];
  /* outputs (caller-owned) */
  double* f_out[RESNMTF_GROUP_MAX_VIEWS];          /* n x k, normalised (output_f) */
  double* s_out[RESNMTF_GROUP_MAX_VIEWS];          /* k x k (output_s) */
  double* g_out[RESNMTF_GROUP_MAX_VIEWS];          /* m x k (output_g) */
  double* lambda_out[RESNMTF_GROUP_MAX_VIEWS];     /* k */
  double* mu_out[RESNMTF_GROUP_MAX_VIEWS];         /* k */
  double* all_error;                     /* err_capacity entries; the first *iters_done are written */
  int err_capacity;                      /* >= n_iters (fixed count, capped by max_iters) or max_iters (convergence) */
  int* iters_done;
} resnmtf_group_job;
int resnmtf_group_run(int device_id, int n_jobs, const resnmtf_group_job* jobs, double tol, int max_iters);

/*
 * One factorisation in fp64 at any size: res_nmtf_inner (R/main.r:32-140) for one job, spread over the whole device.
 * The job, its outputs, n_iters, tol and max_iters mean what they mean for resnmtf_group_run, and the arithmetic is that
 * entry's own -- update_matrices (R/update_steps.r:272-319) view by view in index order with the association orders
 * (X G) S^T, (F S) ((G^T G) S^T), (F^T X) G, the branch tests, NaN -> 1 in the unrestricted branches only,
 * star_prod_relevant through the row / column maps, update_lm, abs; calculate_error as the explicit residual
 * ||X - (F S) G^T||_F^2 / ||X||_F^2 (R/utils.r:157-166) averaged over the views; the loop of R/main.r:53-80 and
 * normalisation_check (R/utils.r:176-195) -- only its distribution differs: a sweep of a view is a short sequence of
 * ordinary launches on one stream (tall-skinny products on the fp64 MFMA, row-local updates, k x k jobs), so there is no
 * cap on n_rows * n_cols and k goes to RESNMTF_MAX_K.  No atomics and no waiting between workgroups; every sum has an order
 * fixed by the job's shapes and k, so two calls give the same bits (not the bits of resnmtf_group_run: the orders differ).
 * In convergence mode (n_iters == 0) the sweep's mean error is read back after every sweep and the stop rule is applied
 * on the host; the state returned is the stop sweep's.
 * Blocking; no handle: the call selects device_id, sizes one device buffer (two padded fp64 images of every view, the
 * factors, two scratch matrices, product slabs, partials, the error history, the maps) before any launch and refuses
 * with RESNMTF_ERR_ALLOC, the byte count in resnmtf_last_error(NULL), when it exceeds the free device memory.
 * Refused before any device work (RESNMTF_ERR_INVALID), with resnmtf_group_run's texts: job NULL, a struct_size
 * mismatch, max_iters < 1, tol not finite, n_views outside [1, 8], k outside [1, 64] or above a view dimension, NULL
 * input or output pointers, non-finite inputs, negative restriction entries or a non-zero diagonal, an index pair
 * outside its views, n_iters < 0, err_capacity below the sweeps allowed.  A refusal writes no output.
 * DESIGN.md section 21.
 */
int resnmtf_fp64_run(int device_id, const resnmtf_group_job* job, double tol, int max_iters);

/*
 * The launch geometry resnmtf_fp64_run takes for an n_rows x n_cols view at k -- a function of these three numbers alone.
 * out[RESNMTF_FP64_PLAN_INTS]: the padded k (16 / 32 / 48 / 64); then row tiles, contraction splits and contraction
 * indices per split of the X G product, of the X^T F product, and (64-row tiles, column splits, columns per split) of
 * the residual; last the leading dimensions of the fp64 images of X and of X^T (rows padded to 32, kept off the multiples
 * of 1024).  A split count above 1 means partial products in a slab, summed in split order by the consumer.
 * Refused (RESNMTF_ERR_INVALID): out NULL, a dimension below 1, k outside [1, 64] or above a dimension.  No device work.
 */
#define RESNMTF_FP64_PLAN_INTS 12
int resnmtf_fp64_plan(int n_rows, int n_cols, int k, int* out);

/*
 * resnmtf_fp64_run with sparse views, stored sparse and streamed sparse.  View v is sparse when
 * sp->view[v].col_ptr is not NULL: the 0-based canonical CSC of the PRE-PROCESSED view (what R/utils.r:416-422 leaves of
 * it: non-negative, column-normalised; the reference densifies a sparse Matrix with as.matrix, R/utils.r:416-419, and so
 * factorises the matrix these arrays stand for).  job->x[v] must then be NULL; a view with both, or with neither, is
 * refused.  Dense and sparse views mix freely; with sp NULL or no sparse view the call is resnmtf_fp64_run, bit for bit.
 * Everything else about the job -- limits, outputs, n_iters, tol, max_iters, restrictions, maps, refusal texts -- is
 * resnmtf_fp64_run's.
 * A sparse view keeps no fp64 image on the device: a CSC copy for X^T F and a CSR copy for X G (built on the host by a
 * counting sort, a row's entries in ascending column order), int64 pointers, int32 indices, fp64 values -- 24 bytes per
 * stored entry plus the pointers.  update_f / update_g (R/update_steps.r:141-207) get their products from an fp64 SpMM
 * over a row-major copy of the other factor: one lane group per line, fma in ascending entry order; a line longer than
 * 256 entries is cut into at most 16 pieces of equal length, summed in piece order.  update_s (R/update_steps.r:220-240)
 * is unchanged.  calculate_error (R/utils.r:157-166) of a sparse view is the trace form
 *   (||X||^2 - 2 <S, (F^T X) G> + <((F^T F) S) (G^T G), S>) / ||X||^2
 * from the k x k matrices of the view's own sweep step (no pass over X; within 1e-15 of the explicit residual); a dense
 * view of the same job keeps the explicit residual.  ||X||^2 is summed over the stored values (R/main.r:48).  Same
 * determinism as resnmtf_fp64_run: no atomics, orders fixed by the structure and k, two calls give the same bits.
 * Refused before any device work (RESNMTF_ERR_INVALID): an sp->struct_size mismatch, and per sparse view what
 * resnmtf_set_view_csc refuses on the host -- col_ptr[0] != 0, col_ptr not monotone, a row index out of range or not
 * strictly increasing within a column, a non-finite or negative value, NULL row_idx / values.  The one device buffer is
 * sized before any launch and refused with RESNMTF_ERR_ALLOC and its byte count.  A refusal writes no output.
 */
typedef struct resnmtf_fp64_sparse_view {   /* 0-based canonical CSC of the pre-processed view; all NULL = dense view */
  const long long* col_ptr;                 /* n_cols + 1 */
  const int* row_idx;                       /* strictly ascending within a column */
  const double* values;                     /* finite, >= 0 */
} resnmtf_fp64_sparse_view;
typedef struct resnmtf_fp64_sparse {
  int struct_size;                          /* sizeof the struct */
  resnmtf_fp64_sparse_view view[RESNMTF_GROUP_MAX_VIEWS];
} resnmtf_fp64_sparse;
int resnmtf_fp64_run_sparse(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                            double tol, int max_iters);

/*
 * How resnmtf_fp64_run_sparse streams an n_rows x n_cols sparse view of this structure at k -- a function of the
 * structure and k alone, never of the device.  out[RESNMTF_FP64_SPARSE_PLAN_INTS]: the padded k (16 / 32 / 48 / 64);
 * for the X G product (lines = rows) the split count, the entries per piece and the longest line; the same three for
 * X^T F (lines = columns); last the lines one 64-lane wave owns (64 / padded k, one above 32).  There is one form: every
 * line piece is owned by one lane group.  A split count above 1: pieces in a slab, summed in piece order by the update.
 * Refused (RESNMTF_ERR_INVALID): out NULL, a dimension below 1, k outside [1, 64] or above a dimension, and the
 * structural refusals of resnmtf_fp64_run_sparse.  No device work.
 */
#define RESNMTF_FP64_SPARSE_PLAN_INTS 8
int resnmtf_fp64_sparse_plan(int n_rows, int n_cols, int k, const long long* col_ptr, const int* row_idx, int* out);

/*
 * resnmtf_fp64_run_sparse with views, initial factors and results in DEVICE memory.  With dev NULL
 * the call is resnmtf_fp64_run_sparse: the same launches, the same bits.  Every result is BIT FOR BIT that of the host
 * route on the same values: widening fp32 / fp16 / bf16 to fp64 is exact, the two padded images of a device view are byte
 * for byte those the host loops build, and the column sums keep the host loop's order.
 *   x[v]        a dense view in device memory: a resnmtf_device_matrix, its ptr NULL when not given, of any of the four dtypes and
 *               any strides >= 0 (0: an expanded tensor); job->x[v] must then be NULL.  One kernel reads it once and writes
 *               both images.  Host dense views, device dense views and host sparse views mix in one job; a view given in
 *               two places, or in none, is refused.  The values of a device view are not validated.
 *   f0 / s0 / g0 [v]   initial factors in device memory, n x k, k x k, m x k: all three of a view, or none of them (then the
 *               job's host pointers are read); with them job->f0[v], s0[v], g0[v], lambda0[v] and mu0[v] must be NULL.
 *   lambda0 / mu0 [v]  k x 1 (col_stride is not read); only beside device factors.  ptr NULL: the column sums of F0 / G0,
 *               one accumulator per column from 0.0 over ascending rows, as the host route sums them.
 *   f_out ... mu_out   device double*, column-major contiguous (as resnmtf_get_factors_device writes): all five of every
 *               view of the job, or none.  With them the job's five host output pointers may be NULL (one that is set is
 *               still written) and nothing of size n or m is downloaded.  all_error and iters_done stay host pointers.
 *   state_f ... state_mu   optional, all five of every view or none: the RAW state after the last sweep, before
 *               normalisation_check, copied device to device on the run's stream -- what a later call resumes from.
 *   stream      as for resnmtf_set_view_device: an event is recorded there and the run's stream waits for it.  The call
 *               blocks until every output is written, so the sources may be freed on return.
 * Refused before any allocation or launch (RESNMTF_ERR_INVALID), the text naming the view and the field: a struct_size
 * mismatch, a device view or factor given beyond n_views, the both / neither / partial cases above, an unknown dtype, a
 * negative stride, a pointer that is not device memory of device_id, a matrix that reaches beyond its allocation.
 */
typedef struct resnmtf_fp64_device {
  int struct_size;                                         /* sizeof the struct */
  void* stream;
  resnmtf_device_matrix x[RESNMTF_GROUP_MAX_VIEWS];
  resnmtf_device_matrix f0[RESNMTF_GROUP_MAX_VIEWS], s0[RESNMTF_GROUP_MAX_VIEWS], g0[RESNMTF_GROUP_MAX_VIEWS];
  resnmtf_device_matrix lambda0[RESNMTF_GROUP_MAX_VIEWS], mu0[RESNMTF_GROUP_MAX_VIEWS];
  double *f_out[RESNMTF_GROUP_MAX_VIEWS], *s_out[RESNMTF_GROUP_MAX_VIEWS], *g_out[RESNMTF_GROUP_MAX_VIEWS];
  double *lambda_out[RESNMTF_GROUP_MAX_VIEWS], *mu_out[RESNMTF_GROUP_MAX_VIEWS];
  double *state_f[RESNMTF_GROUP_MAX_VIEWS], *state_s[RESNMTF_GROUP_MAX_VIEWS], *state_g[RESNMTF_GROUP_MAX_VIEWS];
  double *state_lambda[RESNMTF_GROUP_MAX_VIEWS], *state_mu[RESNMTF_GROUP_MAX_VIEWS];
} resnmtf_fp64_device;
int resnmtf_fp64_run_device(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                            const resnmtf_fp64_device* dev, double tol, int max_iters);

/*
 * resnmtf_fp64_run_device with SPARSE views in device memory -- what torch's sparse_csc, sparse_csr
 * and (coalesced) sparse_coo tensors hold, for data produced on the device (the reference densifies a sparse Matrix with
 * as.matrix, R/utils.r:416-419, and res_nmtf_inner, R/main.r:32-140, factorises the matrix these arrays stand for).  With
 * spd NULL the call is resnmtf_fp64_run_device: the same launches, the same bits.
 *   view[v]     layout, index_type, dtype, ptr_or_rows, idx_or_cols, values and nnz as resnmtf_set_view_sparse_device takes
 *               them: contiguous 0-based arrays, entries in ANY order, stored positions distinct (a position stored twice
 *               is refused, nothing is summed), explicit zeros stay stored, the view taken as PRE-PROCESSED (R/utils.r:416-422
 *               done).  A view is given when any of its seven fields is not zero; an all-zero entry is a view that comes
 *               from elsewhere.
 *   stream      as dev->stream: an event is recorded there and the run's stream waits for it.  With dev and spd both
 *               given the two must name the same stream.  The call returns when the outputs are written, so the arrays
 *               may be freed on return.
 * A view's data are in exactly one of four places -- job->x, sp, dev->x, spd --; all four kinds mix in one job.
 * Every result (F, S, G, lambda, mu, All_Error, the sweep count, the raw state) and the plan of the passes are BIT FOR BIT
 * those of resnmtf_fp64_run_sparse on the canonical CSC (columns ascending, rows ascending within a column, explicit zeros
 * kept) of the same (row, column, value widened to fp64) set: widening is exact, the positions are distinct (so their
 * sorted order is unique), the CSR copy is the sort by r m + c (a row's entries in ascending column order, what the
 * host's counting sort gives), and every sum order is a function of the structure alone.
 * Nothing runs per entry on the host and no array of size nnz, n or m crosses the bus for such a view: it is checked and
 * sorted on the device with the kernels of resnmtf_set_view_sparse_device (a CSC input whose rows already ascend strictly
 * within every column skips the first of the two sorts); the host reads back the failure word and the longest row and
 * column.  The canonical arrays are built in transient allocations and copied device to device into the job's buffer:
 * at most 48 bytes per stored entry + 8 (n + m + 2) + 24 bytes + the sort's temporary storage while a view is built, 24
 * bytes per stored entry + 8 (n + m + 2) kept per view until the job's buffer holds it.  Free device memory is checked
 * before each allocation (RESNMTF_ERR_ALLOC, the byte count in resnmtf_last_error(NULL)).
 * Refused before any device work (RESNMTF_ERR_INVALID), the text naming the view: a struct_size mismatch, a view given
 * beyond n_views, a view given in two places or in none, an unknown layout, index type or dtype, nnz < 0, a NULL array
 * (values / idx_or_cols, and COO's rows, may be NULL only when nnz = 0), dev->stream != spd->stream; then per array one
 * that is not device memory of device_id or is shorter than its element count.  Refused by the device checks, with
 * resnmtf_set_view_sparse_device's texts and its lowest-offender rule: pointers that do not start at 0, are not monotone
 * or do not end at nnz; an index out of range; a non-finite or negative value; a position stored twice.  A view without
 * a stored entry does what resnmtf_fp64_run_sparse does with the empty CSC.  A refusal writes no output.
 */
typedef struct resnmtf_fp64_sparse_device_view {
  int layout;                               /* RESNMTF_SPARSE_CSC / _CSR / _COO */
  int index_type;                           /* RESNMTF_INDEX_I32 / _I64, one type for both index arrays */
  int dtype;                                /* RESNMTF_DTYPE_* of values */
  const void* ptr_or_rows;                  /* CSC: n_cols + 1 column pointers; CSR: n_rows + 1 row pointers; COO: nnz rows */
  const void* idx_or_cols;                  /* CSC: nnz row indices; CSR and COO: nnz column indices */
  const void* values;                       /* nnz */
  long long nnz;
} resnmtf_fp64_sparse_device_view;
typedef struct resnmtf_fp64_sparse_device {
  int struct_size;                          /* sizeof the struct */
  void* stream;
  resnmtf_fp64_sparse_device_view view[RESNMTF_GROUP_MAX_VIEWS];
} resnmtf_fp64_sparse_device;
int resnmtf_fp64_run_sparse_device(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                                   const resnmtf_fp64_device* dev, const resnmtf_fp64_sparse_device* spd, double tol,
                                   int max_iters);

/*
 * resnmtf_bisil in DOUBLE precision, without a handle: the per-member silhouettes that
 *     bisilhouette::bisilhouette(data[[i]], row_clustering[[i]], col_clustering[[i]], method = distance)
 * combines into res_nmtf_inner's `bisil` (R/obtain_bicl.r:189-199) and that the k sweep of apply_resnmtf ranks
 * (R/main.r:269-321), computed on the fp64 values of X -- the numbers resnmtf_fp64_run factorised -- where resnmtf_bisil
 * reads a handle's fp32 images.  The definition, the metrics and the layout of the outputs are resnmtf_bisil's; every
 * value is carried in fp64, every sum has resnmtf_bisil's order (no atomics: two calls give equal bits), and on data that
 * fp32 holds exactly the silhouettes are bit for bit resnmtf_bisil's.  Blocking.
 *   n, m, k       the view is n x m, the cluster matrices n x k and m x k; k in [1, 64].
 *   metric        0 = euclidean, 1 = manhattan, 2 = cosine.
 *   x             X in host memory: n x m fp64 column-major, as resnmtf_group_job.x holds a view; copied once into a
 *                 plain n x m fp64 device array (no padded images); or NULL.
 *   x_dev, stream X in device memory: any of the four dtypes, any strides >= 0 (0: an expanded tensor), read where it
 *                 lies after an event recorded on `stream` (the hipStream_t its producer ran on; NULL: the null stream);
 *                 x_dev.ptr NULL when not given.  X is given in exactly one of the two places.
 *   row_clusters, col_clusters   host, column-major 0 / 1 fp64, as resnmtf_bisil takes them.
 *   row_sil, col_sil             host, n x k and m x k column-major, 0 at non-members and inactive biclusters.
 * Per side and active bicluster the restricted block G[f][u] = X(U[u], J_l[f]) is gathered as doubles straight from X --
 * with lanes along the points where the point stride is the smaller one, through a 32 x 32 LDS tile read along the
 * features where the feature stride is --, then the norm, distance and epilogue kernels run on it.
 * Refused before any device work (RESNMTF_ERR_INVALID, text in resnmtf_last_error(NULL)), neither output written: job NULL,
 * a struct_size mismatch, k outside [1, 64], n or m below 1, an unknown metric, X in both places or in neither, NULL
 * cluster or output pointers, an unknown dtype, a negative stride, x_dev.ptr not memory of device_id (or too short for
 * the shape and strides), a cluster entry other than 0 or 1 (resnmtf_bisil's message, that of row_clusters first).
 * The workspace is sized first -- the largest block max_l |J_l| x U_pad doubles, the chunk partials, the lists, the
 * silhouettes and n m doubles for a host X -- and refused with RESNMTF_ERR_ALLOC and its byte count when it exceeds the
 * free device memory.  No active bicluster: zero silhouettes, RESNMTF_OK.
 */
typedef struct resnmtf_fp64_bisil_job {
  int struct_size;                          /* sizeof the struct */
  int n, m, k, metric;
  const double* x;
  resnmtf_device_matrix x_dev;
  void* stream;
  const double *row_clusters, *col_clusters;
  double *row_sil, *col_sil;
} resnmtf_fp64_bisil_job;
int resnmtf_fp64_bisil(int device_id, const resnmtf_fp64_bisil_job* job);

/*
 * How resnmtf_fp64_bisil launches one side of one bicluster (no device work): for |U| = n_u points, n_mem members and k
 * biclusters, and a device X with the given strides, out receives {kq (the per-thread bicluster sums of the distance
 * kernel: 1, 2, 4, 8 or 16), tiles of U per chunk, chunks, the gather form of the row side, of the column side
 * (0 = lanes along the points, 1 = the LDS transpose)}.  A host X has row_stride 1 and col_stride n.
 * Refused (RESNMTF_ERR_INVALID): out NULL, n_u or n_mem below 1, k outside [1, 64], a negative stride.
 */
#define RESNMTF_FP64_BISIL_PLAN_INTS 5
int resnmtf_fp64_bisil_plan(int n_u, int n_mem, int k, long long row_stride, long long col_stride, int* out);

/*
 * resnmtf_fp64_bisil of a SPARSE view, without a handle: the per-member silhouettes behind the
 * `bisil` that res_nmtf_inner attaches to every result (R/obtain_bicl.r:189-199) and that the k sweep of apply_resnmtf
 * ranks (R/main.r:269-321), for a view that resnmtf_fp64_run_sparse or resnmtf_fp64_run_sparse_device factorised -- on the
 * fp64 values that were factorised, where resnmtf_bisil_sparse reads a handle's fp32 values, and without the n x m fp64
 * matrix that resnmtf_fp64_bisil would need of it.  Blocking.
 *   n, m, k, metric, row_clusters, col_clusters, row_sil, col_sil   as in resnmtf_fp64_bisil_job.
 *   x             the view in host memory: the 0-based canonical CSC of the pre-processed view, as resnmtf_fp64_run_sparse
 *                 takes it (col_ptr NULL when not given); or
 *   x_dev, stream the view in device memory, as resnmtf_fp64_run_sparse_device takes it: CSC, CSR or coalesced COO, int32 or
 *                 int64 indices, fp64 / fp32 / fp16 / bf16 values, entries in any order, explicit zeros stay stored (all
 *                 seven fields zero when not given).  The arrays are read where they lie after an event recorded on
 *                 `stream`; nothing of size nnz, n or m of the view crosses the bus.  X is given in exactly one place.
 * The silhouettes are BIT FOR BIT those of resnmtf_fp64_bisil on the densified matrix of the same values widened to fp64,
 * and so, on values fp32 holds exactly, those of resnmtf_bisil_sparse; two calls give equal bits.  Per side and active
 * bicluster the block G, |J_l| x U_pad doubles, is zero-filled and one wave per feature line scatters the stored entries
 * that fall in U into it (the row side from the CSC columns, the column side from the CSR rows; indices within a line are
 * distinct: no atomics); the norm, distance and epilogue kernels of resnmtf_fp64_bisil then run on it unchanged.
 * On the device the view is a CSC and a CSR copy, int64 pointers, int32 indices, fp64 values: 24 bytes per stored entry
 * plus the pointers.  The host route builds the CSR by the counting sort of resnmtf_fp64_run_sparse; the device route
 * checks and sorts the arrays with the kernels of resnmtf_set_view_sparse_device in transient allocations.  Every index
 * is verified before the first scatter is launched.
 * Refused before any device work (RESNMTF_ERR_INVALID, text in resnmtf_last_error(NULL)), neither output written: what
 * resnmtf_fp64_bisil refuses, with its texts -- job NULL, a struct_size mismatch, k outside [1, 64], n or m below 1, an
 * unknown metric, X in both places or in neither, NULL cluster or output pointers, a cluster entry other than 0 or 1 --;
 * for a host view what resnmtf_fp64_run_sparse refuses of view 0 (NULL row_idx / values, col_ptr[0] != 0, col_ptr not
 * monotone, a row index out of range or not strictly increasing within a column, a non-finite or negative value); for a
 * device view what resnmtf_fp64_run_sparse_device refuses of view 0 (an unknown layout, index type or dtype, nnz < 0, a
 * NULL array, an array that is not device memory of device_id or is too short; then, by the device checks, bad pointers,
 * an index out of range, a non-finite or negative value, a position stored twice).
 * The workspace -- the block, the norms, the chunk partials, the silhouettes, the lists, the two rank tables (n + m ints)
 * and the two sparse copies -- is sized first and refused with RESNMTF_ERR_ALLOC and its byte count when it exceeds the
 * free device memory.  No active bicluster: zero silhouettes, RESNMTF_OK, no device work.  A view without a stored entry
 * is scored as the all-zero matrix.
 */
typedef struct resnmtf_fp64_bisil_sparse_job {
  int struct_size;                          /* sizeof the struct */
  int n, m, k, metric;
  resnmtf_fp64_sparse_view x;
  resnmtf_fp64_sparse_device_view x_dev;
  void* stream;
  const double *row_clusters, *col_clusters;
  double *row_sil, *col_sil;
} resnmtf_fp64_bisil_sparse_job;
int resnmtf_fp64_bisil_sparse(int device_id, const resnmtf_fp64_bisil_sparse_job* job);

/*
 * shuffle_view (R/obtain_bicl.r:11-22) of one view in DOUBLE precision, without a handle: the
 * draw that obtain_shuffled_f (R/obtain_bicl.r:31-42) factorises, made of the fp64 values of X -- the numbers
 * resnmtf_fp64_run factorised -- where resnmtf_shuffle_view permutes a handle's fp32 image.  Blocking.
 *   n, m          the view is n x m.
 *   seed          the draw: out[i] = X[pi(i)], i column-major in out, pi(i) row-major in X, pi the Feistel permutation
 *                 of resnmtf_shuffle_view for the same seed (csrc/resnmtf_feistel.h).  Every source value is widened
 *                 to fp64 exactly.
 *   x             X in host memory: n x m fp64 column-major, as resnmtf_group_job.x holds a view; copied once into a
 *                 plain n x m fp64 device array; or NULL.
 *   x_dev, stream X in device memory: any of the four dtypes, any strides >= 0 (0: an expanded tensor), read where it
 *                 lies after an event recorded on `stream` (the hipStream_t its producer ran on; NULL: the null stream);
 *                 x_dev.ptr NULL when not given.  X is given in exactly one of the two places.
 *   out           device memory of device_id owned by the caller: n m doubles, column-major (row stride 1, column
 *                 stride n).  The draw is written there and normalised in place; a device source needs no n m buffer.
 *                 It is written after the same event on `stream`, for a host X too (what the caller enqueued may still
 *                 use the memory), and is complete when the call returns.
 *   n_empty_rows, n_empty_cols   (host, not NULL) the rows / columns of the draw, BEFORE any shift, that sum to exactly
 *                 0.0: the redraw condition of R/obtain_bicl.r:14-18 as resnmtf_view_empty_lines reports it.  The caller
 *                 redraws with another seed; the library does not loop.
 *   row_mask, col_mask           (host, n and m bytes, or NULL) 1 where a line is empty.
 *   normalise     != 0: the non-negativity shift and column normalisation apply_resnmtf applies to shuffled data
 *                 (R/obtain_bicl.r:35 -> R/utils.r:416,422) in fp64, out = (x + shift[c]) / colsum[c]; the column
 *                 minimum and sum in column_stats_kernel's order (lane t of 256 takes rows t, t + 256, ..., then the
 *                 256-wide tree), so that on a source fp32 holds the result rounded to fp32 is bit for bit what
 *                 resnmtf_shuffle_view(normalise = 1) stores.  A column that shifts to all zero gives NaN, as in R.
 *   was_negative  (host, or NULL) with normalise: 1 if an entry was negative (R/utils.r:23-25); 0 without.
 * No floating-point atomics: two calls give equal bits (integer atomics for the two counts alone).
 * Refused before any device work (RESNMTF_ERR_INVALID, text in resnmtf_last_error(NULL)), nothing written: job NULL, a
 * struct_size mismatch, n or m below 1, n m above 2^62 (the Feistel domain), X in both places or in neither, out NULL,
 * n_empty_rows / n_empty_cols NULL, an unknown dtype, a negative stride, x_dev.ptr or out not memory of device_id (or too
 * short for the shape and strides: reaching beyond the allocation the pointer lies in), out overlapping x_dev, device_id
 * out of range.  The n m doubles that stage a host X are refused with RESNMTF_ERR_ALLOC and the byte count when they
 * exceed the free device memory, on the byte count alone: before x or out is looked at.
 */
typedef struct resnmtf_fp64_shuffle_job {
  int struct_size;                          /* sizeof the struct */
  int n, m, normalise;
  unsigned long long seed;
  const double* x;
  resnmtf_device_matrix x_dev;
  void* stream;
  double* out;
  int *was_negative, *n_empty_rows, *n_empty_cols;
  unsigned char *row_mask, *col_mask;
} resnmtf_fp64_shuffle_job;
int resnmtf_fp64_shuffle(int device_id, const resnmtf_fp64_shuffle_job* job);

/*
 * shuffle_view (R/obtain_bicl.r:11-22) of one SPARSE view in DOUBLE precision, without a handle:
 * resnmtf_fp64_shuffle's draw of a view that is stored sparse, made of its stored entries alone -- no n x m array exists
 * at any point.  Blocking.
 *   n, m, seed    as in resnmtf_fp64_shuffle_job: a stored entry at (r, c) with value x lands at
 *                 i = feistel_perm_inverse(r m + c, n m, seed) (csrc/resnmtf_feistel.h), that is column i / n, row i % n,
 *                 with the value x widened to fp64.  Explicit zeros stay stored; the draw holds exactly the source's nnz
 *                 entries.  Positions and values are bit for bit the CSC of resnmtf_fp64_shuffle(normalise = 0) of the
 *                 densified view read at those positions (that draw is +0.0 everywhere else), and on values fp32 holds the
 *                 structure and values of resnmtf_shuffle_view_sparse for the same seed.
 *   x             the view in host memory: the 0-based canonical CSC of the pre-processed view, as resnmtf_fp64_run_sparse
 *                 takes it (col_ptr NULL when not given); or
 *   x_dev, stream the view in device memory, as resnmtf_fp64_run_sparse_device takes it: CSC, CSR or coalesced COO, int32 or
 *                 int64 indices, fp64 / fp32 / fp16 / bf16 values, entries in any order (all seven fields zero when not
 *                 given), read where it lies after an event recorded on `stream`.  X is given in exactly one place.
 *   out_col_ptr, out_row_idx, out_values   device memory of device_id owned by the caller: m + 1 int64, nnz int64 and nnz
 *                 doubles, the canonical CSC of the draw (rows ascending within a column) -- what torch.sparse_csc_tensor
 *                 wraps and what resnmtf_fp64_run_sparse_device reads without its first sort.  Written after the same
 *                 event, complete when the call returns.  out_row_idx / out_values may be NULL when nnz = 0.
 *   n_empty_rows, n_empty_cols   (host, not NULL) the rows / columns of the draw that hold no stored entry > 0.  The
 *                 values are non-negative, so these are the lines that sum to exactly 0.0: the counts and masks
 *                 resnmtf_fp64_shuffle reports on the densified view.  The caller redraws; the library does not loop.
 *   row_mask, col_mask           (host, n and m bytes, or NULL) 1 where a line is empty.
 *   normalise     != 0: out_values[e] = (x + 0.0) / colsum[c] in fp64, colsum[c] summed over the stored entries of the
 *                 column in fp64_shuffle_stats_kernel's order (lane t of 256 adds the entries whose row is = t mod 256 in
 *                 ascending row order from 0.0, then the 256-wide tree).  The absent +0.0 entries change no bit of a
 *                 non-negative sum and the shift of a non-negative column is 0, so the values are bit for bit those of
 *                 resnmtf_fp64_shuffle(normalise = 1) of the densified view at the stored positions whenever that draw has
 *                 no empty column; in an empty column a stored zero gives 0 / 0 = NaN, as there.  (The f32 route,
 *                 resnmtf_shuffle_view_sparse, sums a column in plain entry order: against it the normalised values agree
 *                 to f32 rounding only.)
 * No floating-point atomics: two calls give equal bits (integer atomics for the two counts alone).  A view without a
 * stored entry: zero pointers, every line empty, nothing of size zero is launched.
 * Transient device memory: 68 bytes per stored entry at its peak plus the pointers and masks, sized
 * first and refused with RESNMTF_ERR_ALLOC and its byte count when it exceeds the free device memory.
 * Refused before any device work (RESNMTF_ERR_INVALID, text in resnmtf_last_error(NULL)), nothing written: what
 * resnmtf_fp64_shuffle refuses, with its texts where the condition is the same -- job NULL, a struct_size mismatch, n or m
 * below 1, n m above 2^62, X in both places or in neither, NULL outputs or counts, device_id out of range, an output that is
 * not memory of device_id or too short, outputs that overlap each other or x_dev's arrays --; for a host view what
 * resnmtf_fp64_run_sparse refuses of view 0, for a device view what resnmtf_fp64_run_sparse_device refuses of view 0, with
 * their texts (the device checks -- bad pointers, an index out of range, a non-finite or negative value, a position stored
 * twice -- run before any output is written).
 */
typedef struct resnmtf_fp64_shuffle_sparse_job {
  int struct_size;                          /* sizeof the struct */
  int n, m, normalise;
  unsigned long long seed;
  resnmtf_fp64_sparse_view x;
  resnmtf_fp64_sparse_device_view x_dev;
  void* stream;
  long long *out_col_ptr, *out_row_idx;
  double* out_values;
  int *n_empty_rows, *n_empty_cols;
  unsigned char *row_mask, *col_mask;
} resnmtf_fp64_shuffle_sparse_job;
int resnmtf_fp64_shuffle_sparse(int device_id, const resnmtf_fp64_shuffle_sparse_job* job);

/*
 * The sub-sample of stability_repeat (R/stability_analysis.r:124, :184, :232, :238: data[[i]][row_samples, col_samples])
 * of one view in DOUBLE precision, without a handle: out[i, j] = X[rows[i], cols[j]] on the fp64
 * values of X, where resnmtf_subsample_view gathers a handle's fp32 image.  Blocking.
 *   n, m          the source view is n x m.
 *   n_sub, m_sub  the sub-sample is n_sub x m_sub, 1 <= n_sub <= n, 1 <= m_sub <= m.
 *   rows, cols    (host) n_sub / m_sub indices, 0-based, in any order, each at most once: destination row i is source
 *                 row rows[i], destination column j source column cols[j].
 *   x             X in host memory: n x m fp64 column-major; copied once into a plain n x m fp64 device array; or NULL.
 *   x_dev, stream X in device memory: any of the four dtypes, any strides >= 0, read where it lies after an event recorded
 *                 on `stream` (NULL: the null stream) and widened to fp64 exactly; x_dev.ptr NULL when not given.  X is
 *                 given in exactly one of the two places.
 *   out           device memory of device_id owned by the caller: n_sub m_sub doubles, column-major (row stride 1, column
 *                 stride n_sub); written after the same event, complete when the call returns.  The values are carried
 *                 over as they are: NOT re-normalised.
 *   n_empty_rows, n_empty_cols   (host, not NULL) the rows / columns of the sub-sample that sum to exactly 0.0.  One
 *                 running fp64 sum per line in resnmtf_view_empty_lines' order -- a row: destination columns ascending;
 *                 a column: destination rows ascending -- so on any data fp32 holds, mixed signs included, the flags
 *                 are those resnmtf_subsample_view + resnmtf_view_empty_lines report.
 *   row_mask, col_mask           (host, n_sub and m_sub bytes, or NULL) 1 where a line is empty.
 * No floating-point atomics: two calls give equal bits (integer atomics for the two counts alone).
 * Refused before any device work (RESNMTF_ERR_INVALID, text in resnmtf_last_error(NULL)), nothing written: job NULL, a
 * struct_size mismatch, n or m below 1, n_sub / m_sub outside [1, n] / [1, m], rows / cols NULL, X in both places or in
 * neither, out NULL, n_empty_rows / n_empty_cols NULL, an unknown dtype, a negative stride, an index out of range or one
 * that occurs twice (its position named), device_id out of range, x_dev.ptr or out not memory of device_id (or reaching
 * beyond the allocation the pointer lies in), out overlapping x_dev.  The n m doubles that stage a host X are refused with
 * RESNMTF_ERR_ALLOC and the byte count when they exceed the free device memory, on the byte count alone.
 */
typedef struct resnmtf_fp64_subsample_job {
  int struct_size;                          /* sizeof the struct */
  int n, m, n_sub, m_sub;
  const int *rows, *cols;
  const double* x;
  resnmtf_device_matrix x_dev;
  void* stream;
  double* out;
  int *n_empty_rows, *n_empty_cols;
  unsigned char *row_mask, *col_mask;
} resnmtf_fp64_subsample_job;
int resnmtf_fp64_subsample(int device_id, const resnmtf_fp64_subsample_job* job);

/*
 * How resnmtf_fp64_subsample launches (no device work): for a source with the given strides in elements, out receives
 * {the gather form (0 = lanes along the destination rows, 1 = the padded LDS tile transpose; a host X has row_stride 1
 * and col_stride n), the destination rows per workgroup of form 0, the tile edge of form 1, the rows per workgroup of the
 * row sums, the rows and the columns of the column sums' LDS tile}.
 * Refused (RESNMTF_ERR_INVALID): out NULL, a negative stride.
 */
#define RESNMTF_FP64_SUBSAMPLE_PLAN_INTS 6
int resnmtf_fp64_subsample_plan(long long row_stride, long long col_stride, int* out);

/*
 * The sub-sample of stability_repeat (R/stability_analysis.r:124, :184, :232, :238) of one SPARSE view in DOUBLE precision,
 * without a handle: resnmtf_fp64_subsample's gather of a view that is stored sparse, made of its
 * stored entries alone -- no n x m array exists at any point.  Blocking.
 *   n, m, n_sub, m_sub, rows, cols   as in resnmtf_fp64_subsample_job: destination row i is source row rows[i], destination
 *                 column j source column cols[j].  A stored entry survives iff its row is in rows and its column in cols;
 *                 its value is carried as it is, widened to fp64 exactly, NOT re-normalised; explicit zeros
 *                 stay stored.
 *   x             the view in host memory: the 0-based canonical CSC of the pre-processed view, as resnmtf_fp64_run_sparse
 *                 takes it (col_ptr NULL when not given); or
 *   x_dev, stream the view in device memory, as resnmtf_fp64_run_sparse_device takes it: CSC, CSR or coalesced COO, int32 or
 *                 int64 indices, fp64 / fp32 / fp16 / bf16 values, entries in any order (all seven fields zero when not
 *                 given), read where it lies after an event recorded on `stream`.  X is given in exactly one place.
 *   out_col_ptr, out_row_idx, out_values, out_capacity   device memory of device_id owned by the caller: m_sub + 1 int64,
 *                 and out_capacity int64 and out_capacity doubles, of which the first nnz_sub are written: the canonical
 *                 CSC of the sub-sample (rows ascending within a column) -- what torch.sparse_csc_tensor wraps and what
 *                 resnmtf_fp64_run_sparse_device reads without its first sort.  Written after the same event, complete
 *                 when the call returns.  out_row_idx / out_values may be NULL when out_capacity = 0.
 *                 COUNT MODE: all three NULL and out_capacity 0 -- nothing is sorted or written to the caller's device
 *                 memory; nnz_sub, the two counts and the masks are still delivered.
 *   nnz_sub       (host, not NULL) the stored entries of the sub-sample.
 *   n_empty_rows, n_empty_cols   (host, not NULL) the rows / columns of the sub-sample that hold no stored entry > 0.  The
 *                 values are non-negative, so these are the lines that sum to exactly 0.0: the counts and masks
 *                 resnmtf_fp64_subsample reports on the densified view.
 *   row_mask, col_mask           (host, n_sub and m_sub bytes, or NULL) 1 where a line is empty.
 * Structure, values, counts and masks are bit for bit resnmtf_fp64_subsample of the densified view read at the stored
 * positions (+0.0 everywhere else) and, on values fp32 holds, resnmtf_subsample_view_sparse with resnmtf_view_empty_lines.
 * No floating-point arithmetic and no floating-point atomics: two calls give equal bits (integer atomics for the two
 * counts alone); no workgroup waits on another.  A sub-sample without a stored entry: zero pointers, every line empty,
 * nothing of size zero is launched.
 * Transient device memory: 12 bytes per stored entry (48 while a view in device memory is checked
 * and sorted) and 64 per kept entry while the sub-sample is sorted, plus the pointers, the lists and the masks; sized
 * first on min(nnz, n_sub m_sub) kept entries and refused with RESNMTF_ERR_ALLOC and its byte count when it exceeds the
 * free device memory.
 * Refused before any device work (RESNMTF_ERR_INVALID, text in resnmtf_last_error(NULL)), nothing written: what
 * resnmtf_fp64_subsample refuses of the extents and the lists, with its texts -- job NULL, a struct_size mismatch, n or m
 * below 1, n_sub / m_sub outside [1, n] / [1, m], rows / cols NULL, an index out of range or one that occurs twice --; what
 * resnmtf_fp64_shuffle_sparse refuses of the source and the outputs, with its texts -- X in both places or in neither, in
 * fill mode out_col_ptr NULL (or out_row_idx / out_values NULL with out_capacity > 0), counts or nnz_sub NULL, device_id
 * out of range, an output that is not memory of device_id or too short, outputs that overlap each other or x_dev's arrays,
 * and of a host view what resnmtf_fp64_run_sparse refuses of view 0, of a device view what
 * resnmtf_fp64_run_sparse_device refuses of view 0 (the device checks -- bad pointers, an index out of range, a non-finite
 * or negative value, a position stored twice -- run before any output is written) --; a negative out_capacity.
 * out_capacity < nnz_sub is known only after the counting pass: RESNMTF_ERR_INVALID, the text names both numbers, *nnz_sub
 * is set so that the caller can allocate again, nothing else is written.
 */
typedef struct resnmtf_fp64_subsample_sparse_job {
  int struct_size;                          /* sizeof the struct */
  int n, m, n_sub, m_sub;
  const int *rows, *cols;
  resnmtf_fp64_sparse_view x;
  resnmtf_fp64_sparse_device_view x_dev;
  void* stream;
  long long *out_col_ptr, *out_row_idx;
  double* out_values;
  long long out_capacity;
  long long* nnz_sub;
  int *n_empty_rows, *n_empty_cols;
  unsigned char *row_mask, *col_mask;
} resnmtf_fp64_subsample_sparse_job;
int resnmtf_fp64_subsample_sparse(int device_id, const resnmtf_fp64_subsample_sparse_job* job);

/*
 * relevance_results (R/stability_analysis.r:45-67, with jaccard_main :16-33) of cluster matrices that are in device
 * memory, without a handle: the sub-sample's clusters against the reference clusters gathered
 * through the sub-sample's index lists.  Blocking.
 *   n, m, n_sub, m_sub, rows, cols   as in resnmtf_fp64_subsample_job.
 *   k, k_ref      the clusters of the sub-sample / of the reference, each in [1, 64].
 *   row_c, col_c  the sub-sample's clusters, n_sub x k and m_sub x k, in device memory: entries 0 / 1 in any of the four
 *                 dtypes, any strides >= 0 (what resnmtf_fp64_run_device leaves as its row_clusters / col_clusters).
 *   true_r / true_r_dev, true_c / true_c_dev   the reference's clusters, n x k_ref and m x k_ref: each either a host array
 *                 of doubles, column-major, or a device matrix (ptr NULL when not given); exactly one of the two.
 *   stream        the hipStream_t the device matrices' producer ran on (NULL: the null stream).
 *   relevance     (host) k_ref doubles: relevance[j] = max_i I / U with I = |R_i ^ TR_j| |C_i ^ TC_j| and
 *                 U = |R_i| |C_i| + |TR_j| |TC_j| - I in int64, one fp64 division, 0 when U = 0.  Decided on the row
 *                 clusters alone: when exactly one of row_c / true_r has no non-empty column every value is 0, when
 *                 neither has every value is 1.  (true_r counts as gathered: its rows `rows` alone.)
 * Integer atomics only: two calls give equal bits.
 * Refused (RESNMTF_ERR_INVALID, text in resnmtf_last_error(NULL)), relevance not written: job NULL, a struct_size
 * mismatch, bad extents, k or k_ref outside [1, 64], NULL lists or outputs, a reference in both places or in neither, an
 * unknown dtype, a negative stride, an index out of range or twice, device_id out of range, a matrix that is not memory of
 * device_id (or reaches beyond its allocation), and -- found on the device for matrices there -- an entry other than
 * 0 or 1, the matrix and the lowest offending (row, column) in column-major order named.
 */
typedef struct resnmtf_fp64_relevance_job {
  int struct_size;                          /* sizeof the struct */
  int n, m, n_sub, m_sub, k, k_ref;
  resnmtf_device_matrix row_c, col_c;
  const double *true_r, *true_c;
  resnmtf_device_matrix true_r_dev, true_c_dev;
  const int *rows, *cols;
  void* stream;
  double* relevance;
} resnmtf_fp64_relevance_job;
int resnmtf_fp64_relevance(int device_id, const resnmtf_fp64_relevance_job* job);

/*
 * init_mats_inner (R/update_steps.r:78-125) for every view of a job in DOUBLE precision, without a handle (DESIGN.md
 * section 32): the start of the fp64 path on the fp64 values of the views, where resnmtf_init_svd starts from their f32
 * images.  The algorithm is resnmtf_init_svd's, constant for constant: a randomized subspace iteration with
 * L = min(64, 16 ceil((k + 8) / 16)) columns, n_power rounds (below 1: 3), CholeskyQR2 after every product but the last
 * with the 1e-14 trace ridge in round 0 and the 2e-14 trace column cut in both, the L x L eigenproblem of Z^T Z,
 * U = Q Ut, V = Z Ut Sigma^-1; the exact Gram of the short side when min(n, m) < L; then |U|, |V|, the constant unit
 * vector for a zero one, S0 = (|diag(d)| + |N(0, sigma)|) swept by the column sums, F0 and G0 divided by them, lambda0
 * and mu0 their sums.  Omega and the noise of view v come from std::mt19937_64(seed[v]) with std::normal_distribution in
 * resnmtf_init_svd's draw order: the same seed is the same sketch on both routes.
 *   job, sp, dev, spd   where the views' data are, exactly as resnmtf_fp64_run_sparse_device takes them (sp, dev and spd
 *               may be NULL): of the job n_views, k, n_rows, n_cols and x are read, of dev its stream and x, nothing else
 *               (no factors, restrictions, maps or run outputs).  A dense view goes through the two padded fp64 images
 *               and the products of the run, a sparse view through its CSC + CSR copies and the fp64 SpMM passes (no image
 *               is built for it).  The views are done one after another: the transient device memory is one view's.
 *   f0 ... mu0  the outputs per view: F0 (n x k), S0 (k x k), G0 (m x k) column-major, lambda0 and mu0 (k) -- all five
 *               of every view.  outputs_on_device = 0: host pointers; 1: device pointers (contiguous, as resnmtf_fp64_device's
 *               outputs), and then nothing of size n or m crosses the bus.  Both kinds receive the same bits.
 *   singular_values   optional per view (host, k): the k leading singular values.
 *   basis_u / basis_v / basis_d / basis_n_d   optional per view, all four or none (host): the signed vectors the factors
 *               are built from (n x k, m x k, column-major), every singular value the route computed (at most 64,
 *               descending) and their count, as resnmtf_init_svd_basis returns them.
 * The L x L factorisations run on the host in fp64 (at most 64 x 64).  No floating-point atomics and no waiting between
 * workgroups; every sum order is a function of the shapes, k and a sparse view's structure: two calls give the same bits.
 * Blocking.  Refused before any device work (RESNMTF_ERR_INVALID) with the texts of resnmtf_fp64_run_sparse_device for
 * the job and the views' sources, and: init NULL, a struct_size mismatch, sigma negative or not finite, an output missing
 * or given beyond n_views, a basis given in part, a device output that is not memory of device_id.  A view that is all
 * zero or holds a value that is not finite is refused when the device finds it.  A refusal writes no output.
 */
typedef struct resnmtf_fp64_init {
  int struct_size;                          /* sizeof the struct */
  int n_power;                              /* below 1: 3 */
  int outputs_on_device;                    /* 0: f0 ... mu0 are host pointers; 1: device pointers */
  double sigma;                             /* the variance of the noise on S0, >= 0 */
  unsigned long long seed[RESNMTF_GROUP_MAX_VIEWS];
  double *f0[RESNMTF_GROUP_MAX_VIEWS], *s0[RESNMTF_GROUP_MAX_VIEWS], *g0[RESNMTF_GROUP_MAX_VIEWS];
  double *lambda0[RESNMTF_GROUP_MAX_VIEWS], *mu0[RESNMTF_GROUP_MAX_VIEWS];
  double* singular_values[RESNMTF_GROUP_MAX_VIEWS];
  double *basis_u[RESNMTF_GROUP_MAX_VIEWS], *basis_v[RESNMTF_GROUP_MAX_VIEWS], *basis_d[RESNMTF_GROUP_MAX_VIEWS];
  int* basis_n_d[RESNMTF_GROUP_MAX_VIEWS];
} resnmtf_fp64_init;
int resnmtf_fp64_init_svd(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                          const resnmtf_fp64_device* dev, const resnmtf_fp64_sparse_device* spd,
                          const resnmtf_fp64_init* init);

/* ---- phase-level entry points (views sharded one-per-GPU; host does the exchange) ---- */

/* Which image of X the streaming passes of view v use after its upload: *uses_2byte = 0 (f32 images), 1 (fp16) or
 * 2 (uniform 16-bit integers); *rel_error = || X~ - X ||_F / || X ||_F of the 2-byte image (0 when none was built).
 * With x_half = 3 this is the guard's decision (resnmtf_options). */
int resnmtf_view_image_info(resnmtf_handle* h, int v, int* uses_2byte, double* rel_error);

/* The launch plan of view v's two streaming passes, as resnmtf_create / the upload decided it: index [0] = the X.G pass,
 * [1] = the Xt.F pass.  Host only, read-only: no device work, no plan is changed.  The f_chain fields describe the sweep
 * resnmtf_run captured at its latest prepare (prepared = 0: none yet, they read 0).  Refused (RESNMTF_ERR_INVALID): h or
 * out NULL, a bad view, out->struct_size != sizeof(resnmtf_view_plan_info). */
typedef struct resnmtf_view_plan_info {
  int struct_size;         /* = sizeof(resnmtf_view_plan_info), set by the caller */
  int k, kp, nt;           /* k, padded k (16 NT) and 16-column tiles of k */
  int image;               /* what the passes stream: 0 = f32 images, 1 = sparse CSC / CSR, 2 = fp16 image, 3 = 16-bit integer image */
  int kk_mode;             /* k x k hand-off: 0 = mode A (job in workgroup 0), 1 = mode B (aux tiles, last-arriving aux workgroup) */
  int half_unroll;         /* pass_half_kernel wave-steps per trip in effect (2-byte images), else 0 */
  int wide[2];             /* k > 16: 1 = the three-bf16-piece wide form, 0 = the plain f32 MFMA form (and k <= 16) */
  int xcd_order[2];        /* XCD-aware workgroup order in effect (wide form with xcd_order) */
  int waves[2];            /* waves per workgroup */
  int unroll[2];           /* pass_kernel UNROLL (dense f32 images), else 0 */
  int pingpong[2];         /* k <= 16, f32 images: the ping-pong prefetch form */
  int nsplit[2];           /* row splits (slabs) of the contraction */
  int rows_per_split[2];
  int rows[2];             /* contraction rows (X.G: m, Xt.F: n) */
  int rows_pad[2];         /* contraction rows, padded to 64 (X.G: m_pad, Xt.F: n_pad) */
  int short_last[2];       /* the last split is shorter than rows_per_split */
  int ntiles[2];           /* 64-row output tiles (X.G: n_pad / 64, Xt.F: m_pad / 64) */
  int tiles_per_wg[2];     /* wide form: 64-column tiles per workgroup (8 or 4), else 1 */
  int aux_splits[2];       /* mode B: row splits of the aux tiles, else 0 */
  int sparse_blocks[2];    /* sparse view: work blocks of the spmm pass, else 0 */
  int pitch_pad;           /* dense f32 images: 1 = one spare 256-B row per 64-column tile (resnmtf_options.no_pitch_pad = 0) */
  int lds_pad_kb;          /* dense passes: extra LDS per workgroup (resnmtf_options.pass_lds_pad_kb) */
  int prepared;            /* the f_chain fields below are those of the latest prepare */
  int f_chain_hoisted;     /* resnmtf_run runs every F update of a sweep first, in one f_chain_kernel launch */
  int f_chain_views;       /* its view-count instantiation (2, 4 or 8), 0 when not hoisted */
  int f_chain_one_slab;    /* 1: it reads one X.G slab per view (nsplit == 1 everywhere), 0: several */
} resnmtf_view_plan_info;
int resnmtf_view_plan(resnmtf_handle* h, int v, resnmtf_view_plan_info* out);

/* The update side of view v's sweep: which factor_update_kernel<KP, IS_G, NCB, EMIT> instantiation its F and G updates
 * launch and which slab-prefetch depth that instantiation takes at run time, read from the argument blocks of the latest
 * resnmtf_prepare (the ones the launches copy).  Index [0] = the F update, [1] = the G update.  Host only, read-only: no
 * device work, nothing is changed.  Before the first prepare (prepared = 0) the coupling fields (restricted, n_couple,
 * couple_bucket, the map counts, sigma_is_zero, route and the S fields) read 0; the geometry is valid from resnmtf_create on.
 * Refused (RESNMTF_ERR_INVALID): h or out NULL, a bad view, out->struct_size != sizeof(resnmtf_update_plan_info). */
typedef struct resnmtf_update_plan_info {
  int struct_size;         /* = sizeof(resnmtf_update_plan_info), set by the caller */
  int prepared;            /* the coupling fields below are those of the latest prepare */
  int k, kp;               /* k and padded k: the KP of the instantiation */
  int threads;             /* threads per update workgroup */
  int rows_per_group;      /* factor rows a workgroup processes per trip (threads / kp) */
  int emit;                /* 1: the update emits its own fp64 Gram partials (hand-off mode A), 0: mode B */
  int mm64;                /* num and den of a row group on the fp64 MFMA (kp 16, 32, 64), 0: the scalar loop (kp 48) */
  int packk;               /* the bf16 pieces of a row group staged through LDS (kp 32 / 64 without emit) */
  int restricted[2];       /* 1: the coupled formula (no NaN -> 1 guard), 0: the unrestricted form */
  int n_couple[2];         /* coupled views in the numerator: weight != 0, not the view itself, pair not NA */
  int couple_bucket[2];    /* NCB of the instantiation: 0 (unrestricted), 4, 8 or 16 */
  int n_identity_maps[2];  /* of the n_couple views: reached without a map (same names in the same order) ... */
  int n_index_maps[2];     /* ... and through an integer row map */
  int sigma_is_zero[2];    /* the view's own column of phi / psi sums to zero */
  int nsplit[2];           /* slabs of the producing pass the update sums */
  int split_bucket[2];     /* the prefetch depth PF it takes for them: 4, 8 or 16 */
  int rows_per_block[2];   /* factor rows per workgroup (a multiple of rows_per_group) */
  int nblk[2];             /* workgroups of the launch */
  int last_block_rows[2];  /* rows of the last workgroup */
  int route[2];            /* how resnmtf_run's sweep runs this update: 0 = a factor_update_kernel launch, 1 = in the first
                            * workgroups of the pass that consumes it (fuse_updates), 2 = the hoisted f_chain_kernel launch */
  int s_restricted;        /* update_s takes the coupled formula (sum(xi) != 0) */
  int s_n_couple;          /* xi-coupled views in its numerator */
} resnmtf_update_plan_info;
int resnmtf_update_plan(resnmtf_handle* h, int v, resnmtf_update_plan_info* out);

/* Size the per-sweep error buffer for `sweeps` sweeps (phase mode; resnmtf_run sizes it itself).
 * Must precede resnmtf_prepare. */
int resnmtf_reserve_sweeps(resnmtf_handle* h, int sweeps);
/* Validate state, build the device coupling tables, reset the sweep counter and run the first
 * X.G pass of every owned view.  Called implicitly by resnmtf_run.  Asynchronous on the stream. */
int resnmtf_prepare(resnmtf_handle* h);
/* Enqueue one phase of owned view v (asynchronous).  `sweep` is the 0-based index of the sweep being
 * executed since resnmtf_prepare (with slice_p2p it also numbers the arrivals a phase waits for: pass the true count).  Within a sweep the caller visits the owned views in index order:
 * PHASE_F, [exchange F], PHASE_G, [exchange G], PHASE_S, [exchange S].  Exchanges enqueued on the
 * handle's stream are ordered against every kernel that reads or writes the exchanged factor. */
int resnmtf_phase(resnmtf_handle* h, int v, int phase, int sweep);
/* Device address and byte size of a factor of view v (fp64 row-major [len][k]; S is [k][k]).
 * The host may overwrite a mirror (non-owned view) with an exchange enqueued on the handle's
 * stream, or read an owned factor as the source of one (S: after PHASE_S). */
int resnmtf_factor_device_ptr(resnmtf_handle* h, int v, int which, void** ptr, size_t* bytes);
/* Per-view relative errors of sweeps [first, first + count) of an owned view (blocking). */
int resnmtf_view_errors(resnmtf_handle* h, int v, int first, int count, double* out);
int resnmtf_synchronize(resnmtf_handle* h);
/* Accumulated streaming-pass timings (options.time_kernels = 1); reset when reset != 0. */
int resnmtf_pass_timings(resnmtf_handle* h, resnmtf_pass_timing* out, int reset);
/* The same for the other kernels of a view-sharded sweep (options.time_kernels = 1, phase API): summed duration (ms) and
 * launch count per kind -- RESNMTF_TIMED_* below; both arrays have RESNMTF_TIMED_KINDS entries. */
enum { RESNMTF_TIMED_XG = 0, RESNMTF_TIMED_XTF = 1, RESNMTF_TIMED_F_CHAIN = 2, RESNMTF_TIMED_G_CHAIN = 3, RESNMTF_TIMED_S_CHAIN = 4,
       RESNMTF_TIMED_PACK = 5 /* folds, slice pack / unpack */, RESNMTF_TIMED_KINDS = 6 };
int resnmtf_kernel_timings(resnmtf_handle* h, double* ms_total, long long* launches, int reset);

/* Phase API, convergence mode (R/main.r:50-81): tol >= 0 makes every phase enqueued from now on a checked one -- the S chain
 * of a sweep (RESNMTF_PHASE_S_ALL; every rank holds the full per-view error table) evaluates
 * |mean_t - mean_{t-1}| <= tol on the device and sets the stop flag, after which every kernel of the phases returns at
 * once; tol < 0 (default) = fixed sweeps.  Identical bytes on every rank: all ranks stop on the same sweep.
 * resnmtf_loop_state synchronises and reports the sweeps closed since resnmtf_prepare, the flag and the sweep count at
 * which it fired (any pointer may be NULL). */
int resnmtf_set_stop_tolerance(resnmtf_handle* h, double tol);
int resnmtf_loop_state(resnmtf_handle* h, int* sweeps_done, int* done, int* stop_sweep);
/* slice_p2p: the IPC handles of this handle's receive buffers and arrival counters (6 x 64 bytes; *bytes receives the size) /
 * map rank `rank`'s (for the own rank `handles` is ignored).  After every rank is imported the slice phases store to the peers. */
int resnmtf_p2p_export(resnmtf_handle* h, void* handles, size_t capacity, size_t* bytes);
int resnmtf_p2p_import(resnmtf_handle* h, int rank, const void* handles, size_t bytes);
/* slice_p2p: called by every rank at about the same time, after all imports and a host barrier, before resnmtf_prepare.
 * Two rounds of: 1 KB of peer stores into every rank's receive buffers + one arrival on every rank's probe counter; the host
 * polls its counter for the V arrivals; the stream wait the phases use, then a KERNEL reads the stored words (the second
 * round re-reads lines the first left in this device's caches: a wait + launch that does not drop them shows here); an
 * acknowledgement round.  Every wait is a host-side poll bounded by timeout_ms (<= 0: 10 s): nothing can hang.  An error
 * return (text in resnmtf_last_error) means this node cannot run the peer-store exchange: create the handles without it. */
int resnmtf_p2p_selftest(resnmtf_handle* h, int timeout_ms);
/* slice_chains: rows / columns per slice (multiples of 32; slice r covers [r * per_slice, min((r + 1) * per_slice, n))). */
int resnmtf_slice_info(resnmtf_handle* h, int* rows_per_slice, int* cols_per_slice);

#ifdef __cplusplus
}
#endif
#endif /* RESNMTF_HIP_H */
