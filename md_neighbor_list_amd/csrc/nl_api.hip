// nl_api.hip -- host side of libnl_hip.so: the C ABI of include/nl_hip.h over the kernels of nl_kernels.hpp.
// No torch, no CUDA-compat layer: HIP runtime only.  Compiled for gfx950 with -ffp-contract=off.
#include "../../include/nl_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <tuple>
#include <type_traits>
#include <vector>

#include "nl_devbuf.hpp"
#include "nl_kernels.hpp"
#include "nl_stage.hpp"

using namespace nl;

namespace {

// pinned; mirrors the int32 words [status, 16 tickets, pad, total_lo, total_hi] that follow the cell histogram on the
// device; filled by ONE async D2H copy at the end of every build
struct HostResult {
  uint32_t status;
  uint32_t tickets[17];
  uint32_t total_lo, total_hi;
  uint32_t bin_words[2];      // (k_bin_bucket's META_BIN_STATUS / META_BIN_DONE; zero between builds)
  uint32_t kept_lo, kept_hi;  // (copied only by builds that filter: the list total after the stage)
  int64_t total() const { return (int64_t)(((uint64_t)total_hi << 32) | total_lo); }
  int64_t kept() const { return (int64_t)(((uint64_t)kept_hi << 32) | kept_lo); }
};
constexpr int META_TOTAL = 18;  // int32 offset of total_lo from the status word
constexpr int META_FULL27 = 1;  // number of cells the COUNT sweep hands to the batched search (first "ticket" word)
constexpr int META_FILL_LIST = 10;  // number of cells k_fill_masks hands to k_fill_list ("ticket" word 10)
constexpr int META_WORDS = 20;
constexpr int META_KEPT = 22;        // the list total after the filter stage (nl_exclude.inc, nl_types.inc), in the same copy
constexpr int META_WORDS_EXCL = 24;  // (words 20, 21: k_bin_bucket's, META_BIN_STATUS / META_BIN_DONE)
// k_sweep_list_f32 / k_fill_list are launched until this many builds in a row have been enqueued since one was seen to
// hand them cells (and always by a build that runs one again)
constexpr int32_t LIST_QUIET_BUILDS = 4;

// What a build was called with.  A whole-box build has slab == 0, mzl == mz, z_lo == 0.
struct BuildArgs {
  const void* q = nullptr;
  int32_t stride = 4;
  const int32_t* gid = nullptr;
  int32_t n_rows = 0, n = 0;
  int32_t n_ghost_lo = 0;  // slab build: ghosts of the lower layer (the split binning places them in front)
  int32_t z_lo = 0, mzl = 0, slab = 0;
  // nl_make_list_distributed: the ghost counts of the build live on the device (dyn[0], dyn[1]; n is an upper bound);
  // dyn_host: where their pinned copy (words 2, 3) and the exchange's error flags (word 4) arrive with the build's result
  const int32_t* dyn = nullptr;
  const int32_t* dyn_host = nullptr;
  int32_t n_est = 0;  // (dyn) particles expected: owned + the previous build's ghosts; path selection only
  auto tie() const { return std::tie(q, stride, gid, n_rows, n, n_ghost_lo, z_lo, mzl, slab, dyn, dyn_host, n_est); }
  bool operator==(const BuildArgs& o) const { return tie() == o.tie(); }
};

enum Binning : int32_t {
  BINNING_BUCKET,    // one pass into row buckets of cap_row slots (k_bin_bucket)
  BINNING_TWO_PASS,  // row totals, then the scatter (k_bin_rows, k_bin_scatter); split into owned + ghosts for a split slab build
  BINNING_ATOMIC,    // atomic ranks into the cell histogram (k_hash, k_reorder): NL_BINNING=1 and meshes beyond the row tables
};
enum Search : int32_t {
  SEARCH_ROWS,    // fine rows (nl_rows.hpp): fp32, open box
  SEARCH_MASKS,   // COUNT keeps a hit mask per sorted slot (one LDS batch), the expansion writes the list from them
  SEARCH_DENSE,   // hit masks for mask_nb LDS batches per slot, k_fill_dense
  SEARCH_SWEEPS,  // COUNT and FILL distance sweeps
};

// Every choice the launches of a build depend on, made by plan_build.
struct BuildPlan {
  int32_t binning = BINNING_ATOMIC;
  int32_t cap_row = 0;  // BINNING_BUCKET: slots a row
  bool split = false;   // a slab build in two parts (owned rows at PART_BEGIN, ghosts at PART_FINISH)
  int32_t search = SEARCH_SWEEPS;
  int32_t rows_v = 0;   // SEARCH_ROWS: RowsCfg
  int32_t mask_nb = 1;  // mask rows per sorted slot: > 1 for SEARCH_DENSE (and in a fine-row build as dense)
  bool small = false;   // SEARCH_MASKS, fp32 open box, sparse: the 2-wave COUNT (k_sweep_lean_f32) and 1-wave expansion
  bool rows12 = false;  // SEARCH_MASKS: the expansion loads 12 rows a wave up front, not 24
  bool list = true;     // k_sweep_list_f32 / k_fill_list are launched (SEARCH_MASKS: the paths with those two kernels)
  bool full = false;    // full list (both directions), nl_set_list_kind
  bool wide = false;    // key_pointer / base_sorted hold int64 (the list may exceed INT32_MAX entries)
  bool filter = false;  // the filter stage runs: an exclusion table (nl_exclude.inc), a type table (nl_types.inc) or both
  bool images = false;  // the image stage runs behind it (nl_set_pair_images, nl_images.inc)
  int32_t pbc = 0;      // axes of the minimum image (nl_set_periodic_axes)
  int32_t idc = 0;      // SEARCH_MASKS with id classes (k_sweep_class_f32, k_fill_masks<IDC>): C = 2 or 4 classes, 0 = off
  int32_t id_shift = 0; // class of an id: id >> id_shift
  bool cull = false;    // an id-class build with the reach cull (cls_cull; NL_CULL): COUNT leaves cull_bits to the expansion
  bool id_rows = false; // no caller ids, no tilt, the two-level binning: the id of a particle is its input row, so sorted_row
                        // is the compact id array as well (tmp_row and sorted_gid are neither written nor read)
  Box box = {{0, 0, 0}, 0, 0, 0};  // the box of the build (nl_set_box): what its consumers (k_lj, the skin check) fold with
  int32_t tilt = 0;     // box.xy, box.xz or box.yz is not 0: binning and search in sheared coordinates
  bool rerun = false;   // planned as a build that runs one again (finish(), an update's): the profiler plans it that way too
  auto tie() const {
    return std::tie(rerun, binning, cap_row, split, search, rows_v, mask_nb, small, rows12, list, full, wide, filter, images, pbc, idc, id_shift, cull, id_rows,
                    box.L[0], box.L[1], box.L[2], box.xy, box.xz, box.yz, tilt);
  }
  bool operator==(const BuildPlan& o) const { return tie() == o.tie(); }
};

// What a captured graph was captured from (NL_GRAPH): replayed while the key is the same.
struct GraphKey {
  BuildArgs args;
  BuildPlan plan;
  int64_t capacity = 0;
  uint64_t buffers_epoch = 0;
  uint64_t ex_gen = 0;  // generation of the exclusion table (nl_set_exclusions)
  uint64_t ty_gen = 0;  // generation of the type table (nl_set_type_cutoffs)
  int32_t update = 0;   // 1: nl_update_list's chain (check, gated build, snapshot, result copy) ...
  double skin = 0;      // ... and the skin its check was captured with
  auto tie() const { return std::tie(args, plan, capacity, buffers_epoch, ex_gen, ty_gen, update, skin); }
  bool operator==(const GraphKey& o) const { return tie() == o.tie(); }
};

}  // namespace

struct nl_handle_s {
  int dtype = NL_F32, device = 0;
  double rc = 0, L[3] = {0, 0, 0}, rc2 = 0;
  int32_t m[3] = {0, 0, 0};
  int64_t ncell = 0;
  // nl_set_box: the tilt of the triclinic cell b = (xy, Ly, 0), c = (xz, yz, Lz) and its shear in double (Grid::k before
  // the rounding to T); L0 = the box of nl_create (slab and distributed builds need it unchanged)
  double xy = 0, xz = 0, yz = 0, shear[3] = {0, 0, 0}, L0[3] = {0, 0, 0};
  int64_t mesh_cells_cap = 0, mesh_rows_cap = 0;  // cells and rows of x-cells the per-cell / per-row buffers hold
  DevBuf<double> lat_dev;  // [LATTICE_CODES][3] lattice vectors of the box of the next build (Grid::lat, SweepArgs::lat)
  float ims_f[3];
  double ims_d[3];
  float rc2_f = 0;
  float ms_f[3];       // cell edge as the reference's float Vec holds it (neighlist_cpu.hpp:389-391)

  int32_t n_max = 0;
  int64_t capacity = 0;      // list entries (half pairs, or twice as many for a full list)
  bool capacity_user = false;
  int list_kind = NL_LIST_HALF;
  int pbc = 0;               // axes of the minimum image, bit d = axis d (nl_set_periodic_axes); 0 = the open box
  bool local_ids = false;    // nl_set_local_ids: slab builds take no caller ids, and the consumers read their lists

  // device buffers (DevBuf: each owns its allocation and knows the bytes and items it holds; freed with the handle)
  DevBuf<int32_t> rank;
  DevBuf<void> sorted;
  DevBuf<int32_t> sorted_row;
  DevBuf<int32_t> sorted_gid;     // ids in cell order, compact
  DevBuf<int32_t> count;
  DevBuf<void> key_pointer;        // [n_rows + 1] int32 (the reference's type, neighlist_cpu.hpp:29) or, in a wide build, int64
  DevBuf<void> kp_alt;             // key_pointer converted to the other width on demand (nl_get_*_csr / nl_get_*_csr64)
  bool kp_alt_valid = false;
  int offset_width = 0;            // nl_set_offset_width: 0 = by capacity (int64 as soon as the list may exceed INT32_MAX), 32, 64
  DevBuf<int32_t> progress;
  // two-level binning (k_bin_*)
  int32_t* row_count = nullptr;   // [nrows] zeroed per build, then row totals
  DevBuf<int32_t> row_start;      // [nrows + 1]
  DevBuf<int32_t> blk_base;       // [bin_blocks][nrows]
  DevBuf<void> tmp_pos;           // particles grouped by row
  DevBuf<int32_t> tmp_row;
  size_t tmp_slots = 0;           // entries of tmp_pos / tmp_row
  // one-pass binning of a whole build (k_bin_bucket): a bucket of cap_row slots per row of x-cells
  DevBuf<int32_t> row_cursor;     // [my * mz] fill levels of the buckets; zero between builds (k_bin_bucket resets them)
  int bucket_env = 1;             // NL_BIN_BUCKETS=0: always the two-pass binning (same-box A/B)
  int32_t bucket_scale = 1;       // cap_row multiplier: doubled when a row has overflowed its bucket
  bool bucket_off = false;        // the buckets outgrew their memory: the two-pass binning from then on
  int32_t bin_blocks = 0, bin_chunk = 0;
  bool bin_two_level = true;      // NL_BINNING=1 selects the atomic-rank path (k_hash/k_reorder)
  DevBuf<void> base_sorted;        // key_pointer of every sorted slot (mask expansion), same width as key_pointer
  DevBuf<uint32_t> masks;          // [n][64] hit bits of every sorted slot, between COUNT_MASKS and k_fill_masks
  DevBuf<int32_t> full27_list;
  DevBuf<void> resort_buf;         // scratch of nl_resort (32 bytes per particle), allocated on first use
  int rows_env = -1;               // NL_ROWS: -1 (default) = the fine-row search where the 27-cell path would need several LDS batches
                                   // per cell (denser than 40.3 particles per cell), 0 = never, 1..3 = RowsCfg<V - 1> wherever a
                                   // build qualifies (tests), 4 = wherever a build qualifies, RowsCfg by density (sweeps)
  size_t dense_masks_limit = (size_t)64 << 30;  // most memory the mask rows of a dense build may take
  int sweep_variant = 3;           // 1: COUNT + FILL distance sweeps;
                                   // 3 (default): COUNT keeping hit masks + mask expansion
                                   // (2 = persistent LDS-DMA sweeps, 4 / 5 = matrix-core searches: measured slower or a draw
                                   // in round 1 and removed)
  int num_cus = 256;
  DevBuf<unsigned long long> dbg_buf;
  int dbg_flags = 0;  // diagnostics (NL_DEBUG_FLAGS)
  DevBuf<int32_t> cell_count;     // [ncell] followed by the status word
  DevBuf<int32_t> cell_start;     // [ncell + 1]
  DevBuf<int32_t> cls_start;      // id-class builds: [C ncell + 1] first slot of every (cell, class) (k_bin_cells<IDC>)
  int idclass_env = 2;            // NL_IDCLASS: classes of the id-class search where a build qualifies (2 or 4), 0 = never
  DevBuf<uint64_t> cull_bits;     // reach-cull builds: [cells][CULL_WORDS] kept-slot ballots of every cell's stream (cls_cull)
  int cull_env = 1;               // NL_CULL=0: id-class builds without the reach cull
  DevBuf<uint64_t> scan_look;     // k_scan_chained: [scan_blocks] entries + the two counters; all zero between launches
  int32_t scan_blocks = 0;
  DevBuf<int64_t> totals;     // [0] = particles (cell scan), [1] = pairs (row scan)
  uint32_t* status = nullptr;
  DevBuf<int32_t> list;
  // transposed full list (compat output)
  DevBuf<int32_t> t_list;
  DevBuf<int32_t> t_count;
  DevBuf<int32_t> t_cursor;
  int64_t t_rows_cap = 0;
  int32_t t_max = 0;
  bool t_valid = false;

  HostResult* host = nullptr;
  hipStream_t own_stream = nullptr;
  // NL_GRAPH=1 / nl_set_graph: asynchronous builds are replayed from a captured hipGraph (one graph per argument set;
  // re-captured when an argument or any buffer changes).  Saves launch overhead on small systems.
  bool use_graph = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  GraphKey graph_key;
  uint64_t buffers_epoch = 1;  // bumped by every (re)allocation and release of a buffer that builds use
  bool begun = false;  // nl_make_list_slab_begin has run, nl_make_list_slab_finish has not
  hipStream_t last_stream = nullptr;
  hipEvent_t ev[NL_NUM_STAGES + 1] = {};

  // the last build enqueued (adopt_build): its arguments (finish() and the profiler run it again from them) and its plan
  // (how finish(), a refill after growth and the getters read its buffers)
  BuildArgs args;
  BuildPlan plan;
  int32_t list_quiet = 0;    // builds enqueued since one was seen to hand cells to k_sweep_list_f32 / k_fill_list
  int64_t reruns[2] = {0, 0};  // builds run again: [0] a row overflowed its bucket, [1] cells listed without the launches
  bool built = false, pending = false;
  int32_t n = 0, n_rows = 0;  // (a distributed build: n is its upper bound until finish() reads the ghost counts)
  int last_error = NL_OK, last_hip = 0;

  // nl_update_list (nl_skin.inc): the Verlet-skin rebuild decision on the device
  double skin = 0;                 // nl_set_skin
  const uint32_t* gate = nullptr;  // while an update's build is enqueued: k_skin_check's `go` word (every launch waits on it)
  DevBuf<void> snap;               // the caller's positions at the last build an update performed (input order, q's stride)
  DevBuf<uint32_t> skin_words;     // [go, over, ticket, pad, updates (u64), builds (u64)] (SKIN_* in nl_skin.inc)
  bool upd_valid = false;          // the last build was an update's, and nothing that forces a build happened since
  bool last_update = false;        // the build enqueued last is an update's (complete without finish())
  const void* upd_q = nullptr;     // positions, stride and n of that build
  int32_t upd_stride = 0, upd_n = 0;

  // nl_set_exclusions (nl_exclude.inc): pairs left out of the list by a stage behind the search
  DevBuf<int32_t> ex_off;          // the table: [ex_n + 1] row offsets, symmetric, per-row ascending, no duplicates
  DevBuf<int32_t> ex_ids;          // (nullptr: no table)
  int32_t ex_n = 0;                // particle count of the builds it applies to; a global table: its ids, [0, ex_n)
  bool ex_global = false;          // nl_set_exclusions_global: the rows of the table are ids of the list, not input rows
  int64_t ex_unique = 0;           // distinct unordered pairs
  uint64_t ex_gen = 0;             // bumped by a set, a clear or a relabel (part of the graph key)
  bool ex_relabel = false;         // a build ran since the last nl_resort: the next one relabels the tables, if any
  DevBuf<void> kp_pre;             // with a table (either): the offsets and the list the search writes, before the stage
  DevBuf<int32_t> list_pre;        // (one offset array and one list capacity, allocated only while a table is set)

  // nl_set_type_cutoffs (nl_types.inc): the cut-off of a pair from the types of its particles, in the same stage
  DevBuf<int32_t> ty_types;        // [ty_n] types in input order (nullptr: no table)
  DevBuf<void> ty_rc2;             // [NL_MAX_TYPES][NL_MAX_TYPES] thresholds in the position type
  int32_t ty_n = 0, ty_ntypes = 0;
  double ty_rc[NL_MAX_TYPES * NL_MAX_TYPES] = {};  // the caller's rc_ab, [ty_ntypes][ty_ntypes]
  uint64_t ty_gen = 0;             // bumped by a set, a clear or a relabel (part of the graph key)
  DevBuf<void> lj_par;             // nl_set_lj_type_params: [3][NL_MAX_TYPES][NL_MAX_TYPES] 4 eps, sigma^2, rc_force^2 in T
  int32_t lj_ntypes = 0;
  double lj_rcf[NL_MAX_TYPES * NL_MAX_TYPES] = {};  // rc_force_ab, [lj_ntypes][lj_ntypes]
  DevBuf<double> vir_part;         // nl_lj_virial (nl_virial.inc): [NL_VIRIAL_BLOCKS][8] block partials, allocated by the first call

  // A table on a grid uniform in r^2 (nl_table.inc): its knots on the device and its scalars in double (rounded to T at the
  // launches, table_view).
  struct TableSet {
    DevBuf<void> tab;                // [nslots][nknots] knots {V, dV, W, dW} in T; items = its bytes (kept across sets that fit)
    int32_t ntypes = 0, nslots = 0, nknots = 0;  // nknots == 0: not set
    double r_min = 0, r_max = 0;
    double x0 = 0, xc = 0, iD = 0;   // r_min^2, r_max^2 and 1 / D
    int lds_env = 1;                 // NL_TABLE_LDS=0 when it was set: the kernels read it from global memory (tests, same-box A/B)
  };
  // nl_set_pair_table: a tabulated pair potential, {F, dF, U, dU}, a slot per unordered pair of types
  TableSet tb;
  // nl_set_eam (nl_eam.inc): the density table of an embedded-atom potential, {G, dG, f, df}, a slot per type, and behind it
  // in ea.tab [ea.ntypes][ea_nke] embedding knots {E, dE, P, dP} on their own grid, uniform in rho; the pair part is tb
  TableSet ea;
  int32_t ea_nke = 0;
  double ea_rhomax = 0, ea_iDrho = 0;  // rho_max and 1 / Drho
  DevBuf<void> ea_part;            // [3][n_max] rho, fp = F'(rho), Fe = F(rho) of the last EAM call in T, allocated by the first call
  // nl_set_sw (nl_sw.inc): the radial tables of a three-body potential, {G, dG, g, dg}, slot t_i ntypes + t_j, and behind them
  // in sw.tab [ntypes^3] knots {Lambda, -, cos0, -} of [t_i][t_j][t_k]; the pair part is tb
  TableSet sw;
  // nl_set_tersoff (nl_tersoff.inc): the radial tables of a bond-order potential on one grid, {U, dU, u, du}, {Q, dQ, q, dq} and
  // (tf_p) {P, dP, p, dp}, slot t_i ntypes + t_j each, and behind them in tf.tab [ntypes^3] {gamma, -, gc, -}, [ntypes^3]
  // {d2, -, h, -}, [ntypes^2] {beta, -, n, -}, [ntypes^2] {e2, -, e2, -}; the pair part is tb
  TableSet tf;
  bool tf_p = false;
  // nl_set_coulomb_table (nl_coulomb.inc): the charge table, {K, dK, C, dC}, one slot; the pair part is tb
  TableSet cl;
  // nl_set_coul_excl_table (nl_coul_excl.inc): the table of the excluded-pair term, {K, dK, C, dC}, one slot, a grid of its own
  TableSet cx;
  // nl_set_dpd (nl_dpd.inc): the weight table of the DPD pair term, {A, dA, 0, 0}, one slot, a grid of its own (dp.ntypes: the
  // slot parameters'), and behind it in dp.tab [dp_nslots] knots {g, 0, sg, 0} and one knot that holds fin(seed); the pair part is tb
  TableSet dp;
  int32_t dp_nslots = 0;
  double dp_dt = 0;
  uint64_t dp_seed = 0;
  // nl_set_steinhardt (nl_steinhardt.inc): the degree, the neighbour range and whether a 3j table came with them (st_l == 0: not set)
  int32_t st_l = 0;
  double st_rmax = 0;
  bool st_w = false;
  DevBuf<void> st_tab;             // the recurrence table and the 3j table in T, sized for NL_STEIN_MAX_L, allocated by the first set
  DevBuf<void> st_part;            // q_lm [n_max + 16][st_cap_l + 1][2] in T and N_b int32 [n_max + 16] of the last call, allocated by the first call
  int32_t st_cap_l = 0, st_cap_n = 0;  // the l and the n_max st_part was sized for
  int32_t st_last_l = 0;           // the l of the last call (the row length of q_lm); 0: no call yet
  // nl_clusters (nl_cluster.inc): the counters of a call that asks for the summary without the sizes
  DevBuf<int32_t> cc_part;         // int32 [n_max + 16], allocated by the first such call
  int32_t cc_cap_n = 0;            // the n_max it was sized for

  // nl_set_pair_images (nl_images.inc): the periodic image of every entry, written by a stage at the end of the build
  bool pair_images = false;        // the flag: builds run the stage, the handle holds the two buffers below
  DevBuf<uint32_t> images;         // [capacity] int8 {s_a, s_b, s_c, 0} per entry, at the entry's index in `list`
  DevBuf<uint16_t> img_code;       // [n_max] faces and wraps of every particle (k_image_codes)
  DevBuf<uint32_t> img_words;      // [wrapped, ticket, pad, pad] of the stage (IMG_* in nl_images.inc); zero between builds
};

namespace {

#define HIPCHK(h, call)                         \
  do {                                          \
    hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) {                     \
      (h)->last_hip = (int)e_;                  \
      (h)->last_error = NL_ERR_HIP;             \
      return NL_ERR_HIP;                        \
    }                                           \
  } while (0)

int fail(nl_handle_t h, int code) {
  if (h) h->last_error = code;
  return code;
}

// nl_exclude.inc
int launch_exclude(nl_handle_t h, int32_t n_rows, hipStream_t s);
int excl_relabel(nl_handle_t h);
// nl_types.inc
int launch_filter(nl_handle_t h, int32_t n_rows, hipStream_t s);
int types_relabel(nl_handle_t h);
// nl_images.inc
int launch_images(nl_handle_t h, int32_t n_rows, hipStream_t s);

// f(T(), OFF()) with the position type and the offset type of the handle's build.
template <typename F> int dispatch_t_off(nl_handle_t h, F&& f) {
  const bool f32 = h->dtype == NL_F32;
  if (h->plan.wide) return f32 ? f(float(), int64_t()) : f(double(), int64_t());
  return f32 ? f(float(), int32_t()) : f(double(), int32_t());
}
// f(std::true_type or std::false_type) by v
template <typename F> void with_flag(bool v, F&& f) { v ? f(std::true_type()) : f(std::false_type()); }

// What every consumer of the list needs first (nl_lj_forces*, nl_pair_vectors*).  Synchronous: the list must be complete
// (and its build must have succeeded).  enqueue: stream-ordered behind the build instead -- a build, or one the host has
// not seen fail; a pending one must be an update's (a plain asynchronous build may still need finish() to complete its
// list) and enqueued on this stream.  Either way the list's ids must index q: a whole build's, or those of a slab build
// made under nl_set_local_ids (rows of the caller's buffer, ghosts behind the owned rows).  The switch drops the list when it
// changes, so a list that exists was built under the value the handle holds.
int consumer_ready(nl_handle_t h, hipStream_t s, bool enqueue) {
  if (enqueue) {
    if (!h->pending && !h->built) return fail(h, NL_ERR_STATE);
    if (h->pending && (!h->last_update || s != h->last_stream)) return fail(h, NL_ERR_STATE);
  } else if (int rc = nl_synchronize(h)) {
    return rc;
  }
  if ((h->args.slab || h->n_rows != h->n) && (!h->local_ids || h->args.gid || h->args.dyn)) return fail(h, NL_ERR_STATE);
  return NL_OK;
}

// A table that filters builds is set (exclusions, types or both): builds run the filter stage.
bool filter_tables(nl_handle_t h) { return h->ex_ids || h->ty_types; }
// ... and it is one over input rows: whole single-device builds only.  (A global exclusion table alone speaks in the ids
// of the list, and filters slab, id and distributed builds too.)
bool filter_rows_only(nl_handle_t h) { return h->ty_types || (h->ex_ids && !h->ex_global); }
// part: PART_ALL = the whole build; PART_BEGIN = everything that needs the OWNED particles only (slab builds: memset +
// the binning pass over [0, n_rows)); PART_FINISH = the rest (the binning pass over the ghosts, search, scan,
// expansion).  BEGIN + FINISH = ALL for the caller; between the two the halo exchange may still be writing the ghosts.
enum { PART_ALL = 0, PART_BEGIN = 1, PART_FINISH = 2 };

// Not a whole single-device build: a slab, caller ids, a distributed build, or one half of a build in two parts.
bool partial_build(const BuildArgs& a, int part) { return a.slab || a.gid || a.dyn || part != PART_ALL; }
// The exclusion table does not cover a build of n_rows rows: an input-row table is for builds of its own n; a global one
// must hold every row's id, which the host knows where the ids are the rows (caller ids are checked by the stage).
bool excl_refuses(nl_handle_t h, const int32_t* gid, int32_t n_rows) {
  if (!h->ex_ids) return false;
  return h->ex_global ? !gid && n_rows > h->ex_n : n_rows != h->ex_n;
}
// Where the search kernels write the offsets and the list: the getters' buffers, or with a filter table the unfiltered
// ones that the stage compacts from.
void* search_kp(nl_handle_t h) { return h->plan.filter ? h->kp_pre : h->key_pointer; }
int32_t* search_list(nl_handle_t h) { return h->plan.filter ? h->list_pre : h->list; }
// Entries of the last build's list (after the stage, if it ran); growth keeps using the unfiltered total.
int64_t list_total(nl_handle_t h) { return h->plan.filter ? h->host->kept() : h->host->total(); }

// The handle's side of a DevBuf operation: the wrappers below (and follow) are the only places that bump buffers_epoch
// for an allocation, and hip_status the only one that turns its result into last_hip and an nl_status.
int hip_status(nl_handle_t h, hipError_t e) {
  if (e == hipSuccess) return NL_OK;
  (void)hipGetLastError();  // (taken here: the runtime keeps it, and the launch check of the next build would report it)
  h->last_hip = (int)e;
  return fail(h, e == hipErrorOutOfMemory ? NL_ERR_NOMEM : NL_ERR_HIP);
}
// Free, then allocate: the buffer is empty after a failure, and the epoch moves either way.
template <typename T> int dev_alloc(nl_handle_t h, DevBuf<T>& b, size_t bytes, int64_t items = 0) {
  h->buffers_epoch++;  // a captured graph holds the old pointers
  return hip_status(h, b.replace(bytes, items));
}
// Allocate, then free: keeps the old buffer (and the epoch) where the new one cannot be had (nl_set_box: an error
// leaves the handle as it was).
template <typename T> int swap_alloc(nl_handle_t h, DevBuf<T>& b, size_t bytes, int64_t items = 0) {
  const hipError_t e = b.replace_keeping(bytes, items);
  if (e == hipSuccess) h->buffers_epoch++;  // a captured graph holds the old pointers
  return hip_status(h, e);
}
// A buffer that no build touches (scratch of one call, kp_alt, resort_buf, lj_par): no graph of the handle holds it.
template <typename T> int side_alloc(nl_handle_t h, DevBuf<T>& b, size_t bytes) { return hip_status(h, b.replace(bytes)); }

// ---- the stages' buffers, which follow n_max and the list's capacity
constexpr int IMG_WORDS = 4;  // words of h->img_words (IMG_* in nl_images.inc)

// A buffer of `bytes` for `want` items, where it holds fewer (an error leaves it empty: the buffer is not ready).
template <typename T> int follow(nl_handle_t h, DevBuf<T>& b, int64_t want, size_t bytes) {
  if (b.holds(want)) return NL_OK;
  h->buffers_epoch++;  // (as dev_alloc)
  return hip_status(h, b.ensure(want, bytes));
}

// The unfiltered offsets and list while a table filters builds (exclusions, types or both: one offset array, one list
// capacity); nothing without one.
int filter_reserve(nl_handle_t h) {
  if (!filter_tables(h)) return NL_OK;
  if (int rc = follow(h, h->kp_pre, h->n_max, 8 * ((size_t)h->n_max + 32))) return rc;
  return follow(h, h->list_pre, h->capacity, 4 * ((size_t)h->capacity + 16));
}

// The image stage's buffers while the flag is on: one word per entry of the list's capacity, one code per particle of n_max.
int images_reserve(nl_handle_t h) {
  if (!h->pair_images) return NL_OK;
  if (!h->img_words) {
    if (int rc = dev_alloc(h, h->img_words, sizeof(uint32_t) * IMG_WORDS)) return rc;
    HIPCHK(h, hipMemset(h->img_words, 0, sizeof(uint32_t) * IMG_WORDS));
  }
  if (int rc = follow(h, h->img_code, h->n_max, 2 * ((size_t)h->n_max + 64))) return rc;
  return follow(h, h->images, h->capacity, 4 * ((size_t)h->capacity + 16));
}

// Both: wherever n_max or the capacity changes, and again in front of a build (if an allocation failed since).
int stage_reserve(nl_handle_t h) {
  if (int rc = filter_reserve(h)) return rc;
  return images_reserve(h);
}

// The buffers that plan p's stages write through are there.
bool stage_ready(nl_handle_t h, const BuildPlan& p) {
  if (p.filter && !(h->kp_pre.holds(h->n_max) && h->list_pre.holds(h->capacity))) return false;
  if (p.images && !(h->images.holds(h->capacity) && h->img_code.holds(h->n_max) && h->img_words)) return false;
  return true;
}

// The unfiltered buffers, once no table needs them.
void filter_release(nl_handle_t h) {
  h->kp_pre.release(), h->list_pre.release();  // (no epoch here: the callers bump it)
}

void images_release(nl_handle_t h) {
  h->images.release(), h->img_code.release(), h->img_words.release();
  h->buffers_epoch++;
}

// The per-cell and per-row buffers for the handle's mesh (h->m, h->ncell) and n particles: (re)allocated where the mesh needs
// more cells or rows than they hold (nl_initialize allocates them all, nl_set_box only what a larger mesh needs), and cleared:
// the status and meta words sit behind the histogram, at a place that moves with the number of cells, and every word of
// them, of the row cursors and of the scan's look-back array must be zero before a build.
int reserve_mesh(nl_handle_t h, size_t n) {
  int rc;
  const size_t rows_cap = std::max<size_t>((size_t)h->m[1] * h->m[2], (size_t)h->mesh_rows_cap);
  const size_t cells_cap = std::max<size_t>((size_t)h->ncell, (size_t)h->mesh_cells_cap);
  if (rows_cap > (size_t)h->mesh_rows_cap) {
    if ((rc = swap_alloc(h, h->row_start, 4 * (2 * rows_cap + 64)))) return rc;  // (two arrays: a split slab build has two passes)
    if ((rc = swap_alloc(h, h->blk_base, 4 * (rows_cap * (size_t)h->bin_blocks + 16)))) return rc;
    if ((rc = swap_alloc(h, h->row_cursor, 4 * (rows_cap + 16)))) return rc;
  }
  if (cells_cap > (size_t)h->mesh_cells_cap || rows_cap > (size_t)h->mesh_rows_cap) {
    // cells handed from one search kernel to another: half-shell -> 27-cell search, pipelined COUNT -> batched search
    if ((rc = swap_alloc(h, h->full27_list, 4 * (cells_cap + 16)))) return rc;
    if ((rc = swap_alloc(h, h->cell_count, 4 * (cells_cap + 64 + 2 * rows_cap)))) return rc;
    if ((rc = swap_alloc(h, h->cell_start, 4 * (4 * cells_cap + 32)))) return rc;  // (cell_start, or the fine-row table: 4 M + 1)
    if ((rc = swap_alloc(h, h->cls_start, 4 * (4 * cells_cap + 32)))) return rc;   // (the class table: up to 4 M + 1)
    const size_t nblk = std::max<size_t>(n, cells_cap) / SCAN_BLOCK + 2;
    if ((rc = swap_alloc(h, h->scan_look, 8 * (nblk + 1)))) return rc;
    h->scan_blocks = (int32_t)nblk;
  }
  h->mesh_rows_cap = (int64_t)rows_cap, h->mesh_cells_cap = (int64_t)cells_cap;
  h->row_count = h->cell_count + h->ncell + 32;
  h->status = reinterpret_cast<uint32_t*>(h->cell_count + h->ncell);  // cleared by the same memset as the histogram
  h->buffers_epoch++;  // (a captured graph holds the old status address)
  HIPCHK(h, hipMemset(h->row_cursor, 0, 4 * (rows_cap + 16)));
  HIPCHK(h, hipMemset(h->scan_look, 0, 8 * ((size_t)h->scan_blocks + 1)));
  HIPCHK(h, hipMemset(h->cell_count, 0, 4 * (cells_cap + 64 + 2 * rows_cap)));
  return NL_OK;
}

float floor_to_float(double v) {  // largest float <= v
  float f = (float)v;
  if ((double)f > v) f = std::nextafterf(f, -INFINITY);
  return f;
}

int status_to_error(uint32_t st) {
  if (st & ST_OUT_OF_BOX) return NL_ERR_OUT_OF_BOX;
  if (st & ST_DOMAIN) return NL_ERR_DOMAIN;
  if (st & ST_ID_RANGE) return NL_ERR_ARG;  // (a row's id outside the global exclusion table)
  if (st & ST_INDEX_OVERFLOW) return NL_ERR_INDEX_OVERFLOW;
  if (st & ST_CAPACITY) return NL_ERR_CAPACITY;
  return NL_OK;
}

bool has_tilt(nl_handle_t h) { return h->xy != 0 || h->xz != 0 || h->yz != 0; }
Box box_of(nl_handle_t h) { return Box{{h->L[0], h->L[1], h->L[2]}, h->xy, h->xz, h->yz}; }
// lat[3 wr + d] = component d of S(n) = n_a a + n_b b + n_c c for the code wr = (n_a + 1) | (n_b + 1) << 2 | (n_c + 1) << 4
// (lattice_shift in nl_kernels.hpp), in double, in the order of the rule in nl_hip.h (this file is compiled without FMA
// contraction); codes with a field of 3 are never looked up
void lattice_table(const Box& b, double* lat) {
  for (int wr = 0; wr < LATTICE_CODES; wr++) {
    const double na = (wr & 3) - 1, nb = ((wr >> 2) & 3) - 1, nc = ((wr >> 4) & 3) - 1;
    lat[3 * wr + 0] = (na * b.L[0] + nb * b.xy) + nc * b.xz;
    lat[3 * wr + 1] = nb * b.L[1] + nc * b.yz;
    lat[3 * wr + 2] = nc * b.L[2];
  }
}
// The box differs from nl_create's (slab and distributed builds refuse it)
bool box_changed(nl_handle_t h) {
  return has_tilt(h) || h->L[0] != h->L0[0] || h->L[1] != h->L0[1] || h->L[2] != h->L0[2];
}
// A tilt needs both of its axes periodic: xy x and y, xz x and z, yz y and z (NL_ERR_STATE at the build otherwise)
bool tilt_mask_ok(nl_handle_t h) {
  return (h->xy == 0 || (h->pbc & 3) == 3) && (h->xz == 0 || (h->pbc & 5) == 5) && (h->yz == 0 || (h->pbc & 6) == 6);
}

template <typename T> Grid<T> make_grid(nl_handle_t h, const BuildArgs& a, int pbc) {
  Grid<T> g;
  for (int d = 0; d < 3; d++) {
    g.ims[d] = sizeof(T) == 4 ? (T)h->ims_f[d] : (T)h->ims_d[d];
    g.m[d] = h->m[d];
  }
  g.mzl = a.mzl;
  g.slab = a.slab;
  g.z_origin = a.slab ? ((a.z_lo - 1) % h->m[2] + h->m[2]) % h->m[2] : 0;
  g.n_rows = a.n_rows;
  g.pbc = pbc;
  g.dbg = h->dbg_flags;
  g.z_first = a.slab ? a.z_lo - 1 : 0;
  for (int d = 0; d < 3; d++) g.L[d] = (T)h->L[d];
  g.gate = h->gate;
  g.tilt = has_tilt(h) ? 1 : 0;
  for (int d = 0; d < 3; d++) g.k[d] = (T)h->shear[d];
  g.lat = h->lat_dev;
  return g;
}

// exclusive scan of in[n] into out[n+1]; grand total to total[0]
template <typename OFF>
int launch_scan(nl_handle_t h, const int32_t* in, int64_t n, OFF* out, int64_t* total, hipStream_t s,
                uint32_t* total_split = nullptr) {
  if (n <= 0) {  // nothing to scan: out[0] = 0, total = 0 (a zero-size grid is not a valid launch)
    HIPCHK(h, hipMemsetAsync(out, 0, sizeof(OFF), s));
    HIPCHK(h, hipMemsetAsync(total, 0, sizeof(int64_t), s));
    if (total_split) HIPCHK(h, hipMemsetAsync(total_split, 0, 2 * sizeof(uint32_t), s));
    return NL_OK;
  }
  if (n <= SCAN_SMALL_MAX) {  // one launch instead of three (totals of such short arrays fit int32)
    hipLaunchKernelGGL(k_scan_small<OFF>, dim3(1), dim3(1024), 0, s, in, (int32_t)n, total, out, total_split, h->gate);
    return NL_OK;
  }
  const int32_t nb = (int32_t)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
  if (nb > h->scan_blocks) return fail(h, NL_ERR_ARG);  // (sized for max(n_max, cells) in nl_reserve)
  hipLaunchKernelGGL(k_scan_chained<OFF>, dim3(nb), dim3(SCAN_THREADS), 0, s, in, n, h->scan_look, h->scan_blocks, total, out,
                     h->status, total_split, h->gate);
  return NL_OK;
}

// Blocks of a stage kernel whose waves each take one of `units` (rows, or chunks of STAGE_ROWS rows).
int32_t stage_grid(nl_handle_t h, int32_t units) { return std::max(1, std::min((units + 3) / 4, 16 * h->num_cus)); }

// The filter stage on stream s: `count` fills h->count per row, the row scan turns that into key_pointer (its total into
// the meta words, META_KEPT), `compact` copies the kept entries into h->list.  a: the stage's arguments.
template <typename OFF, typename A>
int launch_passes(nl_handle_t h, int32_t n_rows, int32_t units, hipStream_t s, const A& a, void (*count)(A, int32_t*),
                  void (*compact)(A, const OFF*, int32_t*)) {
  const dim3 grid(stage_grid(h, units));
  if (n_rows > 0) hipLaunchKernelGGL(count, grid, dim3(STAGE_THREADS), 0, s, a, h->count);
  if (int rc = launch_scan(h, h->count, n_rows, static_cast<OFF*>(h->key_pointer), h->totals + 2, s, h->status + META_KEPT)) return rc;
  if (n_rows > 0) hipLaunchKernelGGL(compact, grid, dim3(STAGE_THREADS), 0, s, a, static_cast<const OFF*>(h->key_pointer), h->list);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

FastDiv fastdiv_make(uint32_t d) {  // see fastdiv() in nl_kernels.hpp; valid for dividends below 2^31
  FastDiv f;
  f.d = d;
  uint32_t s = 0;
  while ((1ull << s) < d) s++;
  f.s = s;
  f.m = (uint32_t)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
  return f;
}

template <typename T> SweepArgs<T> sweep_args(nl_handle_t h) {
  SweepArgs<T> a;
  a.sorted = static_cast<const Pos<T>*>(h->sorted);
  a.sorted_row = h->sorted_row;
  a.sorted_gid = h->plan.id_rows ? h->sorted_row : h->sorted_gid;
  a.cell_start = h->cell_start;
  a.cls_start = h->cls_start;
  a.mx = h->m[0], a.my = h->m[1], a.mzl = h->args.mzl, a.slab = h->args.slab;
  a.div_mx = fastdiv_make((uint32_t)h->m[0]), a.div_my = fastdiv_make((uint32_t)h->m[1]);
  a.rc2 = sizeof(T) == 4 ? (T)h->rc2_f : (T)h->rc2;
  a.count = h->count;
  a.progress = h->progress;
  a.key_pointer = search_kp(h);
  a.wide = h->plan.wide ? 1 : 0;
  a.n_rows = h->n_rows;
  a.list = search_list(h);
  a.total = h->totals + 1;
  a.capacity = h->capacity;
  a.status = h->status;
  a.masks = h->masks;
  // (the two planes of the hit words, one array each inside the same allocation: 128 + 64 bytes per row)
  a.masks_hi = reinterpret_cast<uint8_t*>(h->masks.get()) + h->masks.bytes() / MASK_ROW_BYTES * MASK_LO_BYTES;
  a.isplit = 1;
  a.mask_nb = h->plan.mask_nb;
  a.full27_list = h->full27_list;
  a.full27_count = reinterpret_cast<int32_t*>(h->status) + META_FULL27;
  a.fill_list_count = reinterpret_cast<int32_t*>(h->status) + META_FILL_LIST;
  a.pbc = h->plan.pbc;
  for (int d = 0; d < 3; d++) a.ms[d] = (T)(h->L[d] / h->m[d]);
  for (int d = 0; d < 3; d++) a.L[d] = (T)h->L[d];
  a.z_origin = h->args.slab ? h->args.z_lo - 1 : 0;
  a.dbg = h->dbg_flags;
  a.dbg_buf = h->dbg_buf;
  a.gate = h->gate;
  a.cull_bits = h->plan.cull ? h->cull_bits.get() : nullptr;
  for (int d = 0; d < 3; d++) a.k[d] = (T)h->shear[d];
  a.lat = h->lat_dev;
  return a;
}

RowsArgs rows_args(nl_handle_t h) {
  RowsArgs a;
  a.sorted = static_cast<const Pos<float>*>(h->sorted);
  a.sorted_row = h->sorted_row, a.sorted_gid = h->plan.id_rows ? h->sorted_row : h->sorted_gid;
  a.fine_start = h->cell_start;
  a.mx = h->m[0], a.my = h->m[1], a.mzl = h->args.mzl, a.slab = h->args.slab;
  a.div_mx = fastdiv_make((uint32_t)h->m[0]), a.div_my = fastdiv_make((uint32_t)h->m[1]);
  a.rc2 = h->rc2_f;
  a.count = h->count;
  a.masks = h->masks;
  a.key_pointer = search_kp(h);
  a.list = search_list(h);
  a.total = h->totals + 1;
  a.capacity = h->capacity;
  a.status = h->status;
  a.over_list = h->full27_list;
  a.over_count = reinterpret_cast<int32_t*>(h->status) + META_FULL27;
  a.wide = h->plan.wide ? 1 : 0;
  a.dbg_buf = h->dbg_buf;
  a.gate = h->gate;
  return a;
}

// The fine-row path (nl_rows.hpp).  V: RowsCfg of the build.
template <int V, bool FULL, typename OFF> void launch_rows(nl_handle_t h, int mode, int32_t ncells, hipStream_t s) {
  const RowsArgs a = rows_args(h);
  const int32_t over_grid = 2 * h->num_cus;
  if (mode == MODE_COUNT) {
    hipLaunchKernelGGL((k_sweep_rows_f32<V, FULL>), dim3(ncells), dim3(ROWS_WAVES * WAVE), 0, s, a);
    hipLaunchKernelGGL((k_rows_overflow<MODE_COUNT, FULL, int32_t>), dim3(over_grid), dim3(ROWS_WAVES * WAVE), 0, s, a);
    return;
  }
  hipLaunchKernelGGL((k_fill_rows<V, FULL, OFF>), dim3(ncells), dim3(ROWS_FW * WAVE), 0, s, a);
  hipLaunchKernelGGL((k_rows_overflow<MODE_FILL, FULL, OFF>), dim3(over_grid), dim3(ROWS_WAVES * WAVE), 0, s, a);
}

// The search of the handle's build (h->plan) in mode MODE_COUNT, or the list expansion behind it in MODE_FILL (which
// finish() launches again after growing the list).  FULL = the list keeps both directions of every pair (the reference
// GPU class's contract); OFF = the type of key_pointer.
template <typename T, bool FULL, bool PBC, typename OFF> void launch_search(nl_handle_t h, int mode, hipStream_t s) {
  const BuildPlan& p = h->plan;
  const int32_t ncells = h->m[0] * h->m[1] * (h->args.slab ? h->args.mzl - 2 : h->args.mzl);  // (the owned layers)
  constexpr bool F32_OPEN = sizeof(T) == 4 && !PBC;
  if (p.search == SEARCH_ROWS) {
    if constexpr (F32_OPEN) {
      if (p.rows_v == 0) launch_rows<0, FULL, OFF>(h, mode, ncells, s);
      else if (p.rows_v == 1) launch_rows<1, FULL, OFF>(h, mode, ncells, s);
      else launch_rows<2, FULL, OFF>(h, mode, ncells, s);
    }
    return;
  }
  const SweepArgs<T> a = sweep_args<T>(h);
  const dim3 cells(ncells), wg(SWEEP_WAVES * WAVE), list_grid(2 * h->num_cus);
  auto count_masks = [&] {  // the COUNT sweep keeping hit masks, for every LDS batch of a cell
    if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((k_sweep_count_masks_f32<FULL, PBC>), cells, wg, 0, s, a);
    else hipLaunchKernelGGL((k_sweep<T, MODE_COUNT_MASKS, FULL, PBC>), cells, wg, 0, s, a);
  };
  switch (p.search) {
    case SEARCH_MASKS:
      if (mode == MODE_COUNT) {
        if constexpr (F32_OPEN) {
          // a workgroup per cell, single-batch cells only; the others go on the hand-over list of the batched search
          constexpr int CAP = SweepCfg<float>::CAP;
          if (p.small && p.id_rows) hipLaunchKernelGGL((k_sweep_lean_f32<FULL, 2, LEAN_SMALL_CAP, true>), cells, dim3(2 * WAVE), 0, s, a);
          else if (p.small) hipLaunchKernelGGL((k_sweep_lean_f32<FULL, 2, LEAN_SMALL_CAP>), cells, dim3(2 * WAVE), 0, s, a);
          else if (!FULL && p.idc == 2) hipLaunchKernelGGL((k_sweep_class_f32<2>), cells, wg, 0, s, a);
          else if (!FULL && p.idc == 4) hipLaunchKernelGGL((k_sweep_class_f32<4>), cells, wg, 0, s, a);
          else if (p.id_rows) hipLaunchKernelGGL((k_sweep_lean_f32<FULL, SWEEP_WAVES, CAP, true>), cells, wg, 0, s, a);
          else hipLaunchKernelGGL((k_sweep_lean_f32<FULL>), cells, wg, 0, s, a);
          if (p.list) hipLaunchKernelGGL((k_sweep_list_f32<FULL>), list_grid, wg, 0, s, a);
        } else {
          count_masks();
        }
        return;
      }
      if (p.small) {  // sparse boxes: a wave per cell (its ~19 rows in one batch), ids of half a stream
        if constexpr (F32_OPEN)
          hipLaunchKernelGGL((k_fill_masks<T, FULL, PBC, OFF, 24, 1, SweepCfg<T>::CAP / 2>), cells, dim3(WAVE), 0, s, a);
      } else if (F32_OPEN && !FULL && p.idc) {
        if constexpr (F32_OPEN && !FULL) {
          constexpr int CAP = SweepCfg<T>::CAP;
          if (p.rows12 && p.idc == 2) hipLaunchKernelGGL((k_fill_masks<T, false, false, OFF, 12, EXPAND_WAVES, CAP, 2>), cells, dim3(EXPAND_WAVES * WAVE), 0, s, a);
          else if (p.rows12) hipLaunchKernelGGL((k_fill_masks<T, false, false, OFF, 12, EXPAND_WAVES, CAP, 4>), cells, dim3(EXPAND_WAVES * WAVE), 0, s, a);
          else if (p.idc == 2) hipLaunchKernelGGL((k_fill_masks<T, false, false, OFF, 24, EXPAND_WAVES, CAP, 2>), cells, dim3(EXPAND_WAVES * WAVE), 0, s, a);
          else hipLaunchKernelGGL((k_fill_masks<T, false, false, OFF, 24, EXPAND_WAVES, CAP, 4>), cells, dim3(EXPAND_WAVES * WAVE), 0, s, a);
        }
      } else if (p.rows12) {
        hipLaunchKernelGGL((k_fill_masks<T, FULL, PBC, OFF, 12>), cells, dim3(EXPAND_WAVES * WAVE), 0, s, a);
      } else {
        hipLaunchKernelGGL((k_fill_masks<T, FULL, PBC, OFF, 24>), cells, dim3(EXPAND_WAVES * WAVE), 0, s, a);
      }
      // cells without masks (a stream of several LDS batches among one-batch neighbours): a second distance search
      if (p.list) hipLaunchKernelGGL((k_fill_list<T, FULL, PBC>), list_grid, wg, 0, s, a);
      return;
    case SEARCH_DENSE:  // mask rows per (slot, LDS batch); list offsets gathered into cell order first
      if (mode == MODE_COUNT) {
        count_masks();
        return;
      }
      if (h->n > 0)
        hipLaunchKernelGGL(k_row_base<OFF>, dim3((h->n + 255) / 256), dim3(256), 0, s, static_cast<const OFF*>(search_kp(h)),
                           h->sorted_row, h->n_rows, h->n, static_cast<OFF*>(h->base_sorted), h->gate);
      hipLaunchKernelGGL((k_fill_dense<T, FULL, PBC, OFF>), cells, dim3(FD_WAVES * WAVE), 0, s, a, static_cast<const OFF*>(h->base_sorted));
      return;
    default:  // SEARCH_SWEEPS
      if (mode == MODE_FILL) hipLaunchKernelGGL((k_sweep<T, MODE_FILL, FULL, PBC>), cells, wg, 0, s, a);
      else if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((k_sweep_count_f32<FULL, PBC>), cells, wg, 0, s, a);
      else hipLaunchKernelGGL((k_sweep<T, MODE_COUNT, FULL, PBC>), cells, wg, 0, s, a);
  }
}

template <typename T, typename OFF> void launch_sweep_kind(nl_handle_t h, int mode, hipStream_t s) {
  const bool pbc = h->plan.pbc != 0;
  if (h->plan.full) pbc ? launch_search<T, true, true, OFF>(h, mode, s) : launch_search<T, true, false, OFF>(h, mode, s);
  else pbc ? launch_search<T, false, true, OFF>(h, mode, s) : launch_search<T, false, false, OFF>(h, mode, s);
}

template <typename T> void launch_sweep(nl_handle_t h, int mode, hipStream_t s) {
  if (h->plan.wide) launch_sweep_kind<T, int64_t>(h, mode, s);
  else launch_sweep_kind<T, int32_t>(h, mode, s);
}

// Mask rows for `nb` LDS batches per particle: allocated on first need (a half-shell handle that meets a minimum-image
// or dense build; a first dense build).
bool mask_rows_ready(nl_handle_t h, int64_t nb, size_t row_bytes = MASK_ROW_BYTES) {
  const size_t need = row_bytes * (size_t)nb * ((size_t)h->n_max + 64);  // (+64: the expansion kernels read whole row batches)
  if (need > h->dense_masks_limit) return false;
  if (need > h->masks.bytes() || !h->masks) return dev_alloc(h, h->masks, need) == NL_OK;
  return true;
}

// The ballot words of a reach-cull build (cls_cull): allocated on first need, and again for a mesh of more cells.
bool cull_bits_ready(nl_handle_t h, int64_t cells) {
  return follow(h, h->cull_bits, cells, sizeof(uint64_t) * CULL_WORDS * (size_t)cells) == NL_OK;
}

// The two-level binning (k_bin_*): meshes of up to BIN_MAX_ROWS rows of x-cells and BIN_MAX_MX cells a row, unless
// NL_BINNING=1 selects the atomic-rank path (k_hash / k_reorder).
bool two_level_ok(nl_handle_t h, int32_t mzl) {
  return h->bin_two_level && (int64_t)h->m[1] * mzl <= BIN_MAX_ROWS && h->m[0] <= BIN_MAX_MX;
}

// The fine-row layout needs the two-level binning (k_bin_cells<FINE>) and a fine table that an int32 can index.
bool rows_layout_ok(nl_handle_t h, int32_t mzl) {
  const int64_t nrows = (int64_t)h->m[1] * mzl;
  return h->bin_two_level && nrows <= BIN_MAX_ROWS && h->m[0] <= BIN_FINE_MAX_MX && 4 * (int64_t)h->m[0] * nrows < 2147483000LL;
}
// Two particles five or more quarter-planes apart along z have rounded products t = z * ims more than 1 apart, so their
// distance along z exceeds ms (1 - 8 m 2^-24) (two roundings of t, relative 2^-24 each, at |t| <= 2 m, and the
// rounding of ims): the pair fails the cut-off test in any rounding of r2 once ms / rc > 1 + 8 m 2^-24 + 2^-20.
bool rows_margin_ok(nl_handle_t h) {
  const double ms = h->L[2] / h->m[2];
  return ms / h->rc >= 1.0 + 8.0 * h->m[2] * 5.9604644775390625e-8 + 9.5367431640625e-7;
}

// Bucket size of the one-pass binning (k_bin_bucket) for a whole build of n particles in my * mzl rows of x-cells, or 0:
// the two-pass binning.  The mean row plus a Poisson-safe margin (BASELINE config 2: 1165 particles a row, sigma 34:
// 1712 slots), times bucket_scale; the buckets (re)allocated on first need, at most 4 n_max + 512 slots a row.
template <typename T> int32_t bucket_cap(nl_handle_t h, int32_t n, int32_t mzl) {
  if (!h->bucket_env || h->bucket_off || !two_level_ok(h, mzl)) return 0;
  const int64_t nrows = (int64_t)h->m[1] * mzl;
  const int64_t cap = (int64_t)h->bucket_scale * ((int64_t)(1.25 * (double)n / (double)nrows) + 256);
  const size_t slots = (size_t)(nrows * cap) + 16;
  if (slots > 4 * ((size_t)h->n_max + 16) + 512 * (size_t)nrows) {
    h->bucket_off = true;
    return 0;
  }
  if (slots > h->tmp_slots) {
    if (dev_alloc(h, h->tmp_pos, sizeof(Pos<T>) * slots) || dev_alloc(h, h->tmp_row, sizeof(int32_t) * slots)) {
      // no room: the two-pass binning, with the buffers it needs
      h->bucket_off = true;
      h->tmp_slots = 0;
      const size_t n_slots = (size_t)h->n_max + 16;
      if (dev_alloc(h, h->tmp_pos, sizeof(Pos<T>) * n_slots) == NL_OK && dev_alloc(h, h->tmp_row, sizeof(int32_t) * n_slots) == NL_OK)
        h->tmp_slots = n_slots, h->last_error = NL_OK;
      return 0;
    }
    h->tmp_slots = slots;
  }
  return (int32_t)cap;
}

// Every choice of a build (BuildPlan) from its arguments and the handle's settings, with the allocations they need (mask
// rows, row buckets; a failed allocation leaves that path out).  part: a slab build in two parts bins its owned rows and
// its ghosts in separate passes.  rerun: a build that runs one again (finish(), an update's build) takes the two-pass
// binning and every launch of its path.
template <typename T> BuildPlan plan_build(nl_handle_t h, const BuildArgs& a, int part, bool rerun) {
  BuildPlan p;
  p.rerun = rerun;
  p.full = h->list_kind == NL_LIST_FULL;
  p.pbc = h->pbc;
  p.box = box_of(h);
  p.tilt = has_tilt(h) ? 1 : 0;
  p.filter = filter_tables(h);
  p.images = h->pair_images;
  // 64-bit list offsets as soon as the list this handle can hold exceeds what an int32 key_pointer can address
  // (the reference's own limit, neighlist_cpu.hpp:15,29); nl_set_offset_width overrides.
  p.wide = h->offset_width == 64 || (h->offset_width == 0 && h->capacity > 2147483647LL);

  // the search, by density: a distributed build's n is an upper bound, n_est what it expects
  const int32_t n = a.dyn ? a.n_est : a.n;
  const int64_t ncl = (int64_t)h->m[0] * h->m[1] * a.mzl;
  const bool variant3 = h->sweep_variant >= 3;
  // Hit masks pay off while a cell's stencil fits one LDS batch; where the mean stencil (27 cells) is close to or
  // beyond the batch size most cells would fall back to a re-search in small batches, so use two full sweeps there.
  const double mean_stream = ncl > 0 ? 27.0 * n / (double)ncl : 0.0;
  const bool sparse_enough = mean_stream <= 0.85 * SweepCfg<T>::CAP;  // mean stencil <= 1088: <= 40.3 per cell
  bool masks = variant3 && sparse_enough && mask_rows_ready(h, 1);
  // The fine-row search (nl_rows.hpp): fp32, open box, the two-level binning, and a cell edge that exceeds the cut-off
  // along z by more than the rounding of the cell hash can hide (rows_margin_ok).  RowsCfg by the mean stencil
  // stream m = 27 <N/cell>: m + 5 sigma within the LDS buffer, the piece a wave walks + 6 sigma within its hit word.
  bool rows = false;
  if (sizeof(T) == 4 && variant3 && p.pbc == 0 && h->rows_env != 0 && rows_layout_ok(h, a.mzl) && rows_margin_ok(h)) {
    int v = -1;
    if (h->rows_env > 0 && h->rows_env <= 3) {
      v = h->rows_env - 1;
    } else if (h->rows_env == 4 || !sparse_enough) {
      // (at the BASELINE densities the 27-cell sweep is the faster one: 0.512 against 0.570 ms at config 2; from 40.3
      // particles per cell on its streams no longer fit one LDS batch: 0.97 against 0.60 ms at rho = 1.1 --
      // profiles/r03_density_sweep.txt)
      // (a wave walks 27 of the 36 windows)
      const double span = mean_stream * 27.0 / 36.0;
      const int cap[3] = {RowsCfg<0>::CAP, RowsCfg<1>::CAP, RowsCfg<2>::CAP}, bits[3] = {16, 32, 32};
      for (int k = 0; k < 3 && v < 0; k++)
        if (mean_stream + 5.0 * std::sqrt(mean_stream) <= cap[k] && span + 6.0 * std::sqrt(span) <= 64.0 * bits[k]) v = k;
    }
    if (v >= 0 && mask_rows_ready(h, 1, v == 0 ? 128 : 256)) rows = true, p.rows_v = v, masks = true;
  }
  if (variant3 && !sparse_enough) {
    // Dense cells: hit masks for up to FD_NB LDS batches per slot instead of a second distance sweep, when the streams
    // (mean + 5 sigma of a Poisson count) fit that many batches and the mask rows fit the memory set aside for them.
    // (Also where the fine rows take the build: mask_nb is what nl_get_build_info reports.)
    const int64_t nb = (int64_t)((mean_stream + 5.0 * std::sqrt(mean_stream) + 64.0) / SweepCfg<T>::CAP) + 1;
    if (nb <= FD_NB && mask_rows_ready(h, nb)) masks = true, p.mask_nb = (int32_t)nb;  // (allocates once)
  }
  p.search = rows ? SEARCH_ROWS : !masks ? SEARCH_SWEEPS : p.mask_nb > 1 ? SEARCH_DENSE : SEARCH_MASKS;
  // sparse boxes (mean stream + 5 sigma within half the LDS buffer: up to 19.6 particles per cell): the 2-wave instance
  // of the lean COUNT sweep, a wave per cell in the expansion; a cell beyond it goes to the batched search like any other
  // that does not fit
  p.small = sizeof(T) == 4 && p.search == SEARCH_MASKS && p.pbc == 0 &&
            mean_stream + 5.0 * std::sqrt(mean_stream) <= (double)LEAN_SMALL_CAP;
  // rows a wave of the expansion loads up front: 24, or 12 where cells hold ~20 particles or fewer (a wave then has ~10
  // rows); from the build's n, which a refill after growth expands again
  p.rows12 = (double)a.n <= 21.0 * (double)std::max<int64_t>(1, ncl);

  // the binning.  A build that can be run again bins in one pass into row buckets, and leaves out the launches for
  // cells whose stencil exceeds the LDS buffer once LIST_QUIET_BUILDS builds in a row have been enqueued without such
  // cells being seen; finish() runs it again without either when a row overflowed its bucket or such a cell was there
  // after all.
  const bool two_level = two_level_ok(h, a.mzl);
  p.split = part != PART_ALL && two_level && a.slab;
  const bool again_ok = !p.split && !a.dyn && !rerun;
  p.list = !again_ok || h->list_quiet < LIST_QUIET_BUILDS;
  p.cap_row = again_ok ? bucket_cap<T>(h, n, a.mzl) : 0;
  p.binning = !two_level ? BINNING_ATOMIC : p.cap_row > 0 ? BINNING_BUCKET : BINNING_TWO_PASS;
  // ids that are input rows: no caller ids (a slab or distributed build passes them), no tilt (a tilted build parks the
  // x-cell in the id slot of tmp and needs tmp_row), the row-wise binning
  p.id_rows = !a.gid && !p.tilt && p.binning != BINNING_ATOMIC;
  // id classes (NL_IDCLASS; k_sweep_class_f32): where they are exact and simple -- the fp32 half list of the one-batch
  // 4-wave path in an open box, ids 0..n-1 (no caller ids), a whole build (no slab, no distributed build), the
  // row-wise binning that writes the class table (k_bin_cells), and a mesh of at least 3 cells a side (27 distinct
  // stencil cells)
  if (sizeof(T) == 4 && p.search == SEARCH_MASKS && !p.small && !p.full && p.pbc == 0 && h->idclass_env > 0 && !a.gid &&
      !a.slab && !a.dyn && !p.split && p.binning != BINNING_ATOMIC && h->m[0] * h->idclass_env <= 4 * BIN_FINE_MAX_MX &&
      h->m[0] >= 3 && h->m[1] >= 3 && a.mzl >= 3 && n > 0) {
    p.idc = h->idclass_env;
    while (((uint32_t)(n - 1) >> p.id_shift) >= (uint32_t)p.idc) p.id_shift++;  // classes [k 2^s, (k + 1) 2^s) cover [0, n)
    p.cull = h->cull_env != 0 && cull_bits_ready(h, ncl);
  }
  return p;
}

BuildPlan plan_for(nl_handle_t h, const BuildArgs& a, int part, bool rerun) {
  return h->dtype == NL_F32 ? plan_build<float>(h, a, part, rerun) : plan_build<double>(h, a, part, rerun);
}

// The build being enqueued, or replayed from a graph, becomes the handle's: finish(), a refill after growth and the
// getters read its buffers by its arguments and plan.
void adopt_build(nl_handle_t h, const BuildArgs& a, const BuildPlan& p) {
  h->args = a;
  h->plan = p;
  h->ex_relabel = true;  // (the cell order nl_resort applies is this build's)
  h->kp_alt_valid = false;
}

// k_bin_bucket / k_bin_scatter keep 8 particles a thread in flight where a chunk is 8 per thread, else 4.  (k_bin_bucket
// in fp32 only: 127 VGPRs; fp64 would spill, and reads its chunk twice instead.)
// The second argument of `launch`: the IDROW instance (BuildPlan::id_rows).
template <typename T, bool BUCKET, typename L> void launch_unrolled(nl_handle_t h, L&& launch) {
  auto by_id = [&](auto u) {
    if (h->plan.id_rows) launch(u, std::true_type());
    else launch(u, std::false_type());
  };
  if constexpr (sizeof(T) == 4 || !BUCKET) {
    if (h->bin_chunk >= 8 * BIN_THREADS) return by_id(std::integral_constant<int, 8>());
  }
  by_id(std::integral_constant<int, 4>());
}

// k_bin_cells: the particles of the rows into cell order, with the fine-row table (FINE) for the fine-row search
template <typename T>
void launch_bin_cells(nl_handle_t h, const Grid<T>& g, int32_t grid, int32_t nrows, const int32_t* row_start, const BinPhase& ph,
                      int32_t cap_row, hipStream_t s) {
  auto launch_as = [&](auto fine, auto idc, auto idrow) {
    hipLaunchKernelGGL((k_bin_cells<T, decltype(fine)::value, decltype(idc)::value, decltype(idrow)::value>), dim3(grid), dim3(256), 0, s, g, nrows, row_start,
                       static_cast<const Pos<T>*>(h->tmp_pos), h->tmp_row, h->cell_start, static_cast<Pos<T>*>(h->sorted),
                       h->sorted_row, h->sorted_gid, ph, cap_row, h->cls_start, h->plan.id_shift);
  };
  auto launch = [&](auto fine, auto idc) {
    if constexpr (decltype(idc)::value > 0) {
      launch_as(fine, idc, std::true_type());  // (an id-class build has no caller ids)
    } else {
      if (h->plan.id_rows) launch_as(fine, idc, std::true_type());
      else launch_as(fine, idc, std::false_type());
    }
  };
  if constexpr (sizeof(T) == 4) {
    if (h->plan.search == SEARCH_ROWS) return launch(std::true_type(), std::integral_constant<int, 0>());
    if (h->plan.idc == 2) return launch(std::false_type(), std::integral_constant<int, 2>());
    if (h->plan.idc == 4) return launch(std::false_type(), std::integral_constant<int, 4>());
  }
  launch(std::false_type(), std::integral_constant<int, 0>());
}

// Enqueues build a along plan p (made by plan_build for these arguments), which becomes the handle's build.
// ev != nullptr: records an event before every stage and one after the last.
template <typename T>
int enqueue_build(nl_handle_t h, const BuildArgs& a, const BuildPlan& p, hipStream_t s, hipEvent_t* ev, int part = PART_ALL) {
  adopt_build(h, a, p);
  if (p.filter && (excl_refuses(h, a.gid, a.n_rows) || (h->ty_types && a.n != h->ty_n) || (filter_rows_only(h) && partial_build(a, part))))
    return fail(h, NL_ERR_STATE);  // (checked by the entry points)
  if (p.images && partial_build(a, part)) return fail(h, NL_ERR_STATE);  // (checked by the entry points)
  if (!stage_ready(h, p)) return fail(h, NL_ERR_NOMEM);  // (the search or a stage would write through a missing buffer)
  if (part != PART_ALL && !p.split) {  // nothing to overlap on this path: BEGIN does nothing, FINISH is the whole build
    if (part == PART_BEGIN) return NL_OK;
    part = PART_ALL;
  }
  const Grid<T> g = make_grid<T>(h, a, p.pbc);
  const int32_t n = a.n, nrows = h->m[1] * a.mzl, my = h->m[1];
  const T* q = static_cast<const T*>(a.q);
  // the three launches of one pass of the two-pass binning; rc_arr / rs_arr: the pass's own row totals and row starts
  auto run_pass = [&](const BinPhase& ph, int32_t* rc_arr, int32_t* rs_arr, int32_t cells_grid, bool events) {
    const int32_t np = ph.i_end - ph.i_beg;
    const int32_t blocks = std::max(1, (np + h->bin_chunk - 1) / h->bin_chunk);  // (an empty pass still publishes its row starts)
    hipLaunchKernelGGL((k_bin_rows<T>), dim3(blocks), dim3(BIN_THREADS), 0, s, q, a.stride, n, h->bin_chunk, g, nrows, rc_arr,
                       h->blk_base, h->status, ph);
    if (events) (void)hipEventRecord(ev[NL_STAGE_CELL_SCAN], s);
    // (no scan launch: every block of k_bin_scatter scans the row totals itself and block 0 publishes the row starts)
    if (events) (void)hipEventRecord(ev[NL_STAGE_REORDER], s);
    launch_unrolled<T, false>(h, [&](auto u, auto idrow) {
      hipLaunchKernelGGL((k_bin_scatter<T, decltype(u)::value, decltype(idrow)::value>), dim3(blocks), dim3(BIN_THREADS), 0, s, q, a.stride, a.gid, n,
                         h->bin_chunk, g, nrows, rc_arr, rs_arr, h->blk_base, static_cast<Pos<T>*>(h->tmp_pos), h->tmp_row,
                         h->status, ph);
    });
    launch_bin_cells<T>(h, g, cells_grid, nrows, rs_arr, ph, 0, s);
  };
  // One allocation = [cell histogram | status, tickets, total (32 words) | row totals]: one memset node clears
  // what this build's path needs (histogram + meta, or meta + row totals); the one-pass binning needs none.
  switch (p.binning) {
    case BINNING_BUCKET: {
      // one pass into the row buckets; k_bin_bucket also starts the meta words and leaves its cursors at zero
      if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_HASH], s));
      const int32_t blocks = std::max(1, (n + h->bin_chunk - 1) / h->bin_chunk);
      launch_unrolled<T, true>(h, [&](auto u, auto idrow) {
        hipLaunchKernelGGL((k_bin_bucket<T, decltype(u)::value, decltype(idrow)::value>), dim3(blocks), dim3(BIN_THREADS), 0, s, q, a.stride, a.gid, n,
                           h->bin_chunk, g, nrows, p.cap_row, h->row_cursor, h->row_start, static_cast<Pos<T>*>(h->tmp_pos),
                           h->tmp_row, h->status);
      });
      if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_CELL_SCAN], s));
      if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_REORDER], s));
      const BinPhase all = {0, n, nrows, 0, 0, 0, nrows, nrows, -1, nullptr};
      launch_bin_cells<T>(h, g, nrows, nrows, h->row_start, all, p.cap_row, s);
      break;
    }
    case BINNING_TWO_PASS:
      if (part == PART_ALL) {
        // (an update's build: k_skin_check has cleared these words where it decided on a build)
        if (!h->gate) HIPCHK(h, hipMemsetAsync(h->cell_count + h->ncell, 0, sizeof(int32_t) * (size_t)(32 + nrows), s));
        if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_HASH], s));
        const BinPhase all = {0, n, nrows, 0, 0, 0, nrows, nrows, -1, a.dyn};
        run_pass(all, h->row_count, h->row_start, nrows, ev != nullptr);
      } else if (part == PART_BEGIN) {
        // owned particles: rows of the layers 1 .. mzl-2, placed behind the n_ghost_lo particles of ghost layer 0
        HIPCHK(h, hipMemsetAsync(h->cell_count + h->ncell, 0, sizeof(int32_t) * (size_t)(32 + 2 * (size_t)nrows), s));
        const BinPhase owned = {0, a.n_rows, nrows, a.n_ghost_lo, a.n_ghost_lo, my, nrows - 2 * my, nrows, -1};
        run_pass(owned, h->row_count, h->row_start, nrows - 2 * my, false);
        HIPCHK(h, hipGetLastError());
        return NL_OK;
      } else {
        // ghosts: layer 0 at the front of the sorted array, layer mzl-1 behind the owned particles
        const BinPhase ghosts = {a.n_rows, n, nrows - my, 0, a.n_rows, 0, my, nrows - my, a.n_ghost_lo};
        run_pass(ghosts, h->row_count + nrows, h->row_start + nrows + 16, 2 * my, false);
      }
      break;
    default: {  // BINNING_ATOMIC
      const int32_t nbp = (n + 255) / 256;
      if (h->gate) {  // an update's build: no memset node, a launch that waits on the decision like the others
        const int64_t words = h->ncell + 32;
        hipLaunchKernelGGL(k_zero_words, dim3((uint32_t)std::min<int64_t>((words + 1023) / 1024, 2048)), dim3(256), 0, s, h->cell_count, words, h->gate);
      } else {
        HIPCHK(h, hipMemsetAsync(h->cell_count, 0, sizeof(int32_t) * (size_t)(h->ncell + 32), s));
      }
      if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_HASH], s));
      if (n > 0) hipLaunchKernelGGL((k_hash<T>), dim3(nbp), dim3(256), 0, s, q, a.stride, n, g, h->cell_count, h->rank, h->status);
      if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_CELL_SCAN], s));
      if (int rc = launch_scan(h, h->cell_count, (int64_t)h->m[0] * h->m[1] * a.mzl, h->cell_start.get(), h->totals, s)) return rc;
      if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_REORDER], s));
      if (n > 0)
        hipLaunchKernelGGL((k_reorder<T>), dim3(nbp), dim3(256), 0, s, q, a.stride, a.gid, n, g, h->cell_start, h->rank,
                           static_cast<Pos<T>*>(h->sorted), h->sorted_row, h->sorted_gid);
    }
  }
  if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_COUNT], s));
  // (rows of particles rejected by the hash keep a stale count: such a build fails with its status anyway)
  launch_sweep<T>(h, MODE_COUNT, s);
  if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_ROW_SCAN], s));
  if (p.wide) {
    if (int rc = launch_scan(h, h->count, a.n_rows, static_cast<int64_t*>(search_kp(h)), h->totals + 1, s, h->status + META_TOTAL)) return rc;
  } else {
    if (int rc = launch_scan(h, h->count, a.n_rows, static_cast<int32_t*>(search_kp(h)), h->totals + 1, s, h->status + META_TOTAL)) return rc;
  }
  if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_FILL], s));
  launch_sweep<T>(h, MODE_FILL, s);
  // the filter tables: the unfiltered list compacted into the getters' buffers (counted in the FILL stage)
  if (p.filter)
    if (int rc = launch_filter(h, a.n_rows, s)) return rc;
  // the image of every entry of the list the getters return (nl_set_pair_images; counted in the FILL stage)
  if (p.images)
    if (int rc = launch_images(h, a.n_rows, s)) return rc;
  if (ev) HIPCHK(h, hipEventRecord(ev[NL_STAGE_TOTAL], s));
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

int enqueue_result_copy(nl_handle_t h, hipStream_t s) {
  const int words = h->plan.filter ? META_WORDS_EXCL : META_WORDS;
  HIPCHK(h, hipMemcpyAsync(h->host, h->status, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, s));
  return NL_OK;
}

int dispatch_build(nl_handle_t h, const BuildArgs& a, const BuildPlan& p, hipStream_t s, hipEvent_t* ev, int part = PART_ALL) {
  return h->dtype == NL_F32 ? enqueue_build<float>(h, a, p, s, ev, part) : enqueue_build<double>(h, a, p, s, ev, part);
}

// Default list capacity (unless the caller fixed it): ideal-gas estimate of the half-pair count
// N * rho * (2/3) pi rc^3 with 30 % head room, twice that for a full list.
int64_t estimate_want(nl_handle_t h) {
  const double rho = (double)h->n_max / (h->L[0] * h->L[1] * h->L[2]);  // (L[0] L[1] L[2]: the volume of a triclinic cell too)
  const double per = rho * (2.0 / 3.0) * 3.14159265358979323846 * h->rc * h->rc * h->rc;
  int64_t want = (int64_t)((double)h->n_max * per * 1.3) + 64 * (int64_t)h->n_max + 4096;
  if (h->list_kind == NL_LIST_FULL) want *= 2;
  return want;
}

int estimate_capacity(nl_handle_t h) {
  if (h->capacity_user) return NL_OK;
  const int64_t want = estimate_want(h);
  if (want > h->capacity) {
    if (int rc = dev_alloc(h, h->list, 4 * (size_t)want)) return rc;
    h->capacity = want;
  }
  return stage_reserve(h);
}

int grow_list(nl_handle_t h, int64_t need) {
  int64_t cap = std::max<int64_t>(need + need / 8 + 1024, h->capacity);
  // a list that an int32 key_pointer can still address stays below the switch to 64-bit offsets
  if (need <= 2147483647LL && cap > 2147483647LL && h->capacity <= 2147483647LL) cap = 2147483647LL;
  int rc = dev_alloc(h, h->list, sizeof(int32_t) * (size_t)cap);
  if (rc) {
    h->capacity = 0;
    return rc;
  }
  h->capacity = cap;
  return stage_reserve(h);
}

// The last build once more, from its own arguments, with the two-pass binning and every launch of its path; waits for it.
int run_again(nl_handle_t h) {
  const BuildArgs a = h->args;
  int rc = dispatch_build(h, a, plan_for(h, a, PART_ALL, true), h->last_stream, nullptr);
  if (!rc) rc = enqueue_result_copy(h, h->last_stream);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->last_stream));
  return NL_OK;
}

// Waits for the pending build; in a synchronous build an undersized list is grown and the fill pass re-run.
int finish(nl_handle_t h, bool may_grow) {
  if (!h->pending) return h->built ? NL_OK : fail(h, NL_ERR_STATE);
  HIPCHK(h, hipStreamSynchronize(h->last_stream));
  h->pending = false;
  uint32_t st = h->host->status;
  {
    // A row past its bucket, or cells handed to k_sweep_list_f32 / k_fill_list by a build that did not launch them: the
    // build is incomplete (whatever else its status says) and runs again without either shortcut.  An overflowed row
    // doubles the buckets of later builds, once; a second overflow ends the one-pass binning for this handle.
    const bool listed = h->plan.search == SEARCH_MASKS &&  // (the path with those two kernels)
                        (h->host->tickets[META_FULL27 - 1] | h->host->tickets[META_FILL_LIST - 1]) != 0;
    const bool overflow = h->plan.cap_row > 0 && (st & ST_ROW_OVERFLOW);
    if (listed) h->list_quiet = 0;
    if (overflow || (listed && !h->plan.list)) {
      if (overflow) h->reruns[0]++, h->bucket_scale *= 2;
      else h->reruns[1]++;
      if (int rc = run_again(h)) return rc;
      st = h->host->status;
    }
  }
  if ((st & ST_INDEX_OVERFLOW) && !(st & ~(ST_CAPACITY | ST_INDEX_OVERFLOW)) && may_grow && !h->plan.wide && h->offset_width == 0) {
    // more than INT32_MAX entries in a build with 32-bit offsets: the list grows past that size, which makes builds of
    // this handle wide (64-bit key_pointer), and the whole build runs again
    int rc = grow_list(h, h->host->total());
    if (rc) return rc;
    if ((rc = run_again(h))) return rc;
    st = h->host->status;
  } else if ((st & ST_CAPACITY) && !(st & ~ST_CAPACITY) && may_grow) {
    int rc = grow_list(h, h->host->total());
    if (rc) return rc;
    // the FILL stage of the build's plan once more (ungated: an update's build is complete by now)
    HIPCHK(h, hipMemsetAsync(h->status, 0, sizeof(uint32_t), h->last_stream));
    if (h->dtype == NL_F32)
      launch_sweep<float>(h, MODE_FILL, h->last_stream);
    else
      launch_sweep<double>(h, MODE_FILL, h->last_stream);
    if (h->plan.filter) rc = launch_filter(h, h->n_rows, h->last_stream);  // (the refilled list is the unfiltered one)
    if (!rc && h->plan.images) rc = launch_images(h, h->n_rows, h->last_stream);  // (into the grown buffer)
    if (!rc) rc = enqueue_result_copy(h, h->last_stream);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->last_stream));
    st = h->host->status;
  }
  int err = status_to_error(st);
  if (h->args.dyn && h->args.dyn_host) {  // a decomposed build: its ghost counts, and whether the exchange held what was sent
    const int32_t* dh = h->args.dyn_host;
    h->n = h->n_rows + dh[2] + dh[3];
    if (!err && dh[4]) err = NL_ERR_CAPACITY;
  }
  h->built = err == NL_OK;
  if (err) return fail(h, err);
  return NL_OK;
}

// The graph of the handle on stream s, captured first (on the private stream: the null stream cannot be captured) from
// what enqueue(stream) enqueues wherever key differs from the key of the graph it holds.
template <typename F> int graph_launch(nl_handle_t h, const GraphKey& key, hipStream_t s, F&& enqueue) {
  if (!h->graph_exec || !(key == h->graph_key)) {
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec), h->graph_exec = nullptr;
    if (h->graph) (void)hipGraphDestroy(h->graph), h->graph = nullptr;
    HIPCHK(h, hipStreamBeginCapture(h->own_stream, hipStreamCaptureModeRelaxed));
    const int rc = enqueue(h->own_stream);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(h->own_stream, &g);
    if (rc) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    HIPCHK(h, e);
    h->graph = g;
    HIPCHK(h, hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
    h->graph_key = key;
  }
  HIPCHK(h, hipGraphLaunch(h->graph_exec, s));
  return NL_OK;
}

}  // namespace

namespace {
template <typename SRC, typename DST>
__global__ void __launch_bounds__(256) k_convert_offsets(const SRC* __restrict__ in, DST* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (DST)in[i];
}

// key_pointer of the last build in the requested width (32 or 64): the buffer the build wrote when the widths agree,
// else a converted copy made once per build.  A wide list that an int32 cannot address is NL_ERR_INDEX_OVERFLOW.
int key_pointer_as(nl_handle_t h, int width, const void** out) {
  const bool want_wide = width == 64;
  if (want_wide == h->plan.wide) {
    *out = h->key_pointer;
    return NL_OK;
  }
  if (!want_wide && list_total(h) > 2147483647LL) return fail(h, NL_ERR_INDEX_OVERFLOW);
  const int64_t cnt = (int64_t)h->n_rows + 1;
  if (!h->kp_alt) {
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = side_alloc(h, h->kp_alt, 8 * ((size_t)h->n_max + 32))) return rc;
    h->kp_alt_valid = false;
  }
  if (!h->kp_alt_valid) {
    const int32_t nb = (int32_t)((cnt + 255) / 256);
    if (want_wide)
      hipLaunchKernelGGL((k_convert_offsets<int32_t, int64_t>), dim3(nb), dim3(256), 0, h->last_stream,
                         static_cast<const int32_t*>(h->key_pointer), static_cast<int64_t*>(h->kp_alt), cnt);
    else
      hipLaunchKernelGGL((k_convert_offsets<int64_t, int32_t>), dim3(nb), dim3(256), 0, h->last_stream,
                         static_cast<const int64_t*>(h->key_pointer), static_cast<int32_t*>(h->kp_alt), cnt);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->last_stream));
    h->kp_alt_valid = true;
  }
  *out = h->kp_alt;
  return NL_OK;
}

// Order-independent checksum of the list: sum over entries (row i, partner j) of mix((id_i << 32) | j), mix(v): v *= 0x9E3779B97F4A7C15,
// v ^= v >> 29 (wrapping) -- the pair-set hash the known answers of SURVEY.md section 8c are stored as.  One wave per row at a time.
template <typename T, typename OFF>
__global__ void __launch_bounds__(256) k_list_checksum(const OFF* __restrict__ kp, const int32_t* __restrict__ list, int32_t n_rows,
                                                       const int32_t* __restrict__ gid, const T* __restrict__ q,
                                                       unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long part[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long h = 0;
  for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < n_rows; row += (int64_t)gridDim.x * 4) {
    uint32_t id = (uint32_t)row;
    if (gid == reinterpret_cast<const int32_t*>(1)) {  // NL_GID_IN_W
      if constexpr (sizeof(T) == 4) id = (uint32_t)__float_as_int(q[(size_t)row * 4 + 3]);
      else id = (uint32_t)__double_as_longlong(q[(size_t)row * 4 + 3]);
    } else if (gid) {
      id = (uint32_t)gid[row];
    }
    const OFF b = kp[row], e = kp[row + 1];
    for (OFF k = b + lane; k < e; k += 64) {
      unsigned long long v = ((unsigned long long)id << 32) | (uint32_t)list[k];
      v *= 0x9E3779B97F4A7C15ULL;
      v ^= v >> 29;
      h += v;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) h += __shfl_xor(h, d, 64);
  if (lane == 0) part[w] = h;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(acc, part[0] + part[1] + part[2] + part[3]);
}

// CopyGather (neighlist_gpu.hpp:144-151) / Gather + SortPtclData (neighlist_cpu.hpp:170-180): dst[s] = src[order[s]]
// for elements of W 32-bit words.
template <int W>
__global__ void __launch_bounds__(256) k_gather_words(const uint32_t* __restrict__ src, const int32_t* __restrict__ order, int32_t n,
                                                      uint32_t* __restrict__ dst) {
  const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t* p = src + (size_t)order[s] * W;
  uint32_t* d = dst + (size_t)s * W;
  if constexpr (W % 4 == 0) {
#pragma unroll
    for (int k = 0; k < W / 4; k++) reinterpret_cast<uint4*>(d)[k] = reinterpret_cast<const uint4*>(p)[k];
  } else if constexpr (W % 2 == 0) {
#pragma unroll
    for (int k = 0; k < W / 2; k++) reinterpret_cast<uint2*>(d)[k] = reinterpret_cast<const uint2*>(p)[k];
  } else {
#pragma unroll
    for (int k = 0; k < W; k++) d[k] = p[k];
  }
}

int get_csr(nl_handle_t h, bool full, int width, const void** key_pointer_dev, const int32_t** list_dev,
            const int32_t** number_of_partners_dev, int64_t* nentries) {
  if (!h) return NL_ERR_ARG;
  int rc = nl_synchronize(h);
  if (rc) return rc;
  if (h->plan.full != full) return fail(h, NL_ERR_STATE);
  if (key_pointer_dev)
    if ((rc = key_pointer_as(h, width, key_pointer_dev))) return rc;
  if (!key_pointer_dev && width == 32 && list_total(h) > 2147483647LL) return fail(h, NL_ERR_INDEX_OVERFLOW);
  if (list_dev) *list_dev = h->list;
  if (number_of_partners_dev) *number_of_partners_dev = h->count;
  if (nentries) *nentries = list_total(h);
  return NL_OK;
}
}  // namespace


extern "C" {

const char* nl_status_string(int s) {
  switch (s) {
    case NL_OK: return "ok";
    case NL_ERR_ARG: return "bad argument";
    case NL_ERR_NOMEM: return "out of memory";
    case NL_ERR_OUT_OF_BOX: return "particle more than one box length outside the box (or NaN)";
    case NL_ERR_CAPACITY: return "pair list capacity exceeded";
    case NL_ERR_HIP: return "HIP runtime error";
    case NL_ERR_STATE: return "call order violated";
    case NL_ERR_MESH: return "fewer than 3 cells along an axis";
    case NL_ERR_INDEX_OVERFLOW: return "more than INT32_MAX list entries behind a 32-bit key_pointer";
    case NL_ERR_NO_DEVICE: return "no usable HIP device";
    case NL_ERR_DOMAIN: return "particle outside the layers declared for this rank";
    case NL_ERR_COMM: return "communication failed (RCCL not loadable, communicator or transport error)";
    default: return "unknown status";
  }
}

int nl_device_count(int* count) {
  if (!count) return NL_ERR_ARG;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *count = c;
  return NL_OK;
}

int nl_create(nl_handle_t* out, int dtype, double rc, double Lx, double Ly, double Lz, int device_id) {
  if (!out) return NL_ERR_ARG;
  *out = nullptr;
  if ((dtype != NL_F32 && dtype != NL_F64) || !(rc > 0) || !(Lx > 0) || !(Ly > 0) || !(Lz > 0)) return NL_ERR_ARG;
  const double L[3] = {Lx, Ly, Lz};
  int32_t m[3];
  for (int d = 0; d < 3; d++) {
    const double r = L[d] / rc;
    if (!(r < 2147483647.0)) return NL_ERR_ARG;
    m[d] = (int32_t)r;  // neighlist_cpu.hpp:384-386
    if (m[d] < 3) return NL_ERR_MESH;
  }
  if ((double)m[0] * m[1] * m[2] > 2.0e9) return NL_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return NL_ERR_NO_DEVICE;
  int dev = device_id;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return NL_ERR_NO_DEVICE;
  if (dev >= ndev) return NL_ERR_ARG;
  if (hipSetDevice(dev) != hipSuccess) return NL_ERR_NO_DEVICE;

  nl_handle_t h = new (std::nothrow) nl_handle_s();
  if (!h) return NL_ERR_NOMEM;
  h->dtype = dtype, h->device = dev, h->rc = rc;
  h->rc2 = rc * rc;  // neighlist_cpu.hpp:394 (double)
  h->rc2_f = floor_to_float(h->rc2);
  for (int d = 0; d < 3; d++) {
    h->L[d] = L[d], h->m[d] = m[d], h->L0[d] = L[d];
    // ms_ and ims_ live in a Vec of the position type (neighlist_cpu.hpp:12,389-391,409-411)
    const float ms_f = (float)(L[d] / m[d]);
    h->ms_f[d] = ms_f;
    h->ims_f[d] = (float)(1.0 / (double)ms_f);
    const double ms_d = L[d] / m[d];
    h->ims_d[d] = 1.0 / ms_d;
  }
  h->ncell = (int64_t)m[0] * m[1] * m[2];
  double lat0[LATTICE_CODES * 3];
  lattice_table(box_of(h), lat0);
  if (h->lat_dev.replace(sizeof(lat0)) != hipSuccess ||
      hipMemcpy(h->lat_dev, lat0, sizeof(lat0), hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&h->host), sizeof(HostResult), hipHostMallocDefault) != hipSuccess) {
    nl_destroy(h);
    return NL_ERR_HIP;
  }
  for (auto& e : h->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      nl_destroy(h);
      return NL_ERR_HIP;
    }
  memset(h->host, 0, sizeof(HostResult));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
    if (const char* v = getenv("NL_SWEEP_VARIANT")) h->sweep_variant = atoi(v) <= 1 ? 1 : 3;
    if (const char* v = getenv("NL_ROWS")) h->rows_env = std::max(-1, std::min(atoi(v), 4));
    if (const char* v = getenv("NL_IDCLASS")) h->idclass_env = atoi(v) >= 4 ? 4 : atoi(v) >= 2 ? 2 : 0;
    if (const char* v = getenv("NL_CULL")) h->cull_env = atoi(v) != 0;
    if (const char* v = getenv("NL_OFFSET_WIDTH")) h->offset_width = atoi(v) == 64 ? 64 : atoi(v) == 32 ? 32 : 0;
    if (const char* v = getenv("NL_BINNING")) h->bin_two_level = atoi(v) != 1;
    if (const char* v = getenv("NL_BIN_BUCKETS")) h->bucket_env = atoi(v) != 0;
    if (const char* v = getenv("NL_GRAPH")) h->use_graph = atoi(v) != 0;
    if (const char* v = getenv("NL_DEBUG_FLAGS")) h->dbg_flags = atoi(v);
  }
  *out = h;
  return NL_OK;
}

int nl_destroy(nl_handle_t h) {
  if (!h) return NL_ERR_ARG;
  (void)hipSetDevice(h->device);
  if (h->pending && h->last_stream) (void)hipStreamSynchronize(h->last_stream);
  if (h->host) (void)hipHostFree(h->host);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
  if (h->graph) (void)hipGraphDestroy(h->graph);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;  // (the device buffers: every DevBuf member frees its own)
  return NL_OK;
}

int nl_initialize(nl_handle_t h, int32_t n_max) {
  if (!h || n_max < 0) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) {
    int rc = finish(h, false);
    (void)rc;
  }
  h->built = false;
  h->upd_valid = false;
  const size_t n = (size_t)n_max;
  const size_t pos_bytes = h->dtype == NL_F32 ? sizeof(Pos<float>) : sizeof(Pos<double>);
  int rc;
  if ((rc = dev_alloc(h, h->rank, 4 * (n + 16)))) return rc;
  if ((rc = dev_alloc(h, h->sorted, pos_bytes * (n + 16)))) return rc;
  if ((rc = dev_alloc(h, h->sorted_row, 4 * (n + 64)))) return rc;  // (+64: k_fill_masks reads whole row batches)
  if ((rc = dev_alloc(h, h->sorted_gid, 4 * (n + 16)))) return rc;
  if ((rc = dev_alloc(h, h->count, 4 * (n + 32)))) return rc;
  // (zero once: a build that leaves out k_sweep_list_f32 -- and then runs again -- scans the stale counts of the cells it
  // listed, which must be counts of earlier builds, never garbage)
  HIPCHK(h, hipMemset(h->count, 0, 4 * (n + 32)));
  if ((rc = dev_alloc(h, h->key_pointer, 8 * (n + 32)))) return rc;  // int32 or int64 offsets (BuildPlan::wide)
  h->kp_alt.release();
  h->kp_alt_valid = false;
  h->resort_buf.release();
  h->ea_part.release();
  // the transposed list and its per-particle counts and cursors (nl_get_full_transposed: sized by n_max on first use)
  h->t_list.release(), h->t_count.release(), h->t_cursor.release();
  h->t_rows_cap = 0;
  if ((rc = dev_alloc(h, h->progress, 4 * (n + 16)))) return rc;
  if ((rc = dev_alloc(h, h->base_sorted, 8 * (n + 64)))) return rc;  // (dense builds only: k_fill_dense)
  // chunk per block: 4096 particles, 8192 from half a million on (cfg 2: binning 60.7 -> 55.9 us, cfg 3 64.7 -> 58.0;
  // 16384: 65.7), more for very large N so that blk_base stays small
  h->bin_chunk = n >= (1 << 19) ? 8192 : 4096;
  if (const char* v = getenv("NL_DEBUG_BIN_CHUNK")) h->bin_chunk = std::max(1024, atoi(v));  // diagnostics
  while ((n + h->bin_chunk - 1) / h->bin_chunk > 1024) h->bin_chunk *= 2;
  h->bin_blocks = (int32_t)((n + h->bin_chunk - 1) / h->bin_chunk);
  if (h->bin_blocks < 1) h->bin_blocks = 1;
  if ((rc = dev_alloc(h, h->tmp_pos, pos_bytes * (n + 16)))) return rc;
  if ((rc = dev_alloc(h, h->tmp_row, 4 * (n + 16)))) return rc;
  h->tmp_slots = n + 16;  // (the buckets of the one-pass binning grow them on first use)
  if (h->sweep_variant >= 3)
    if ((rc = dev_alloc(h, h->masks, (size_t)MASK_ROW_BYTES * (n + 64)))) return rc;
  if ((rc = dev_alloc(h, h->dbg_buf, 8 * (64 + 4 * 4096)))) return rc;
  HIPCHK(h, hipMemset(h->dbg_buf, 0, 8 * (64 + 4 * 4096)));
  if ((rc = dev_alloc(h, h->totals, 8 * 4))) return rc;
  HIPCHK(h, hipMemset(h->totals, 0, 32));
  for (DevBuf<int32_t>* b : {&h->row_start, &h->blk_base, &h->row_cursor, &h->full27_list, &h->cell_count, &h->cell_start, &h->cls_start})
    b->release();  // (all of them anew, without holding the old ones meanwhile)
  h->scan_look.release();
  h->mesh_cells_cap = h->mesh_rows_cap = 0;
  if ((rc = reserve_mesh(h, n))) return rc;
  h->n_max = n_max;
  if ((rc = estimate_capacity(h))) return rc;
  h->t_valid = false;
  return stage_reserve(h);  // (the unfiltered offsets and the particle codes follow n_max)
}

int nl_set_periodic_axes(nl_handle_t h, int mask) {
  if (!h) return NL_ERR_ARG;
  if (mask < 0 || mask > 7) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  h->upd_valid = false;
  if (mask != h->pbc) {
    h->pbc = mask;
    h->built = false;
    h->t_valid = false;
  }
  return NL_OK;
}

int nl_set_box(nl_handle_t h, double Lx, double Ly, double Lz, double xy, double xz, double yz) {
  if (!h) return NL_ERR_ARG;
  const double L[3] = {Lx, Ly, Lz};
  for (double v : {Lx, Ly, Lz, xy, xz, yz})
    if (!std::isfinite(v)) return fail(h, NL_ERR_ARG);
  if (!(Lx > 0) || !(Ly > 0) || !(Lz > 0)) return fail(h, NL_ERR_ARG);
  // the perpendicular widths of the cell (the distances between opposite faces): every axis needs 3 cells of at least rc
  const double sx = (xy * yz - Ly * xz) / (Ly * Lz);
  const double w[3] = {Lx / std::sqrt(1.0 + (xy / Ly) * (xy / Ly) + sx * sx), Ly / std::sqrt(1.0 + (yz / Lz) * (yz / Lz)), Lz};
  int32_t m[3];
  for (int d = 0; d < 3; d++) {
    const double r = w[d] / h->rc;
    if (!(r < 2147483647.0)) return fail(h, NL_ERR_ARG);
    m[d] = (int32_t)r;
  }
  if ((double)m[0] * m[1] * m[2] > 2.0e9) return fail(h, NL_ERR_ARG);
  for (int d = 0; d < 3; d++)
    if (m[d] < 3) return fail(h, NL_ERR_MESH);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  if (Lx == h->L[0] && Ly == h->L[1] && Lz == h->L[2] && xy == h->xy && xz == h->xz && yz == h->yz) return NL_OK;
  // the old box, put back where the new one cannot be had: every step below either succeeds or leaves the buffers usable
  // for the old mesh (swap_alloc keeps a buffer it cannot replace)
  double old_L[3], old_ims_d[3], old_shear[3];
  float old_ms_f[3], old_ims_f[3];
  int32_t old_m[3];
  for (int d = 0; d < 3; d++)
    old_L[d] = h->L[d], old_m[d] = h->m[d], old_ms_f[d] = h->ms_f[d], old_ims_f[d] = h->ims_f[d], old_ims_d[d] = h->ims_d[d],
    old_shear[d] = h->shear[d];
  const double old_tilt[3] = {h->xy, h->xz, h->yz};
  const int64_t old_ncell = h->ncell;
  auto restore = [&](int rc) {
    for (int d = 0; d < 3; d++)
      h->L[d] = old_L[d], h->m[d] = old_m[d], h->ms_f[d] = old_ms_f[d], h->ims_f[d] = old_ims_f[d], h->ims_d[d] = old_ims_d[d],
      h->shear[d] = old_shear[d];
    h->xy = old_tilt[0], h->xz = old_tilt[1], h->yz = old_tilt[2];
    h->ncell = old_ncell;
    if (h->mesh_cells_cap > 0) (void)reserve_mesh(h, (size_t)h->n_max);  // (no allocation: points the status word back, clears)
    double lat[LATTICE_CODES * 3];
    lattice_table(box_of(h), lat);
    (void)hipMemcpy(h->lat_dev, lat, sizeof(lat), hipMemcpyHostToDevice);
    return fail(h, rc);
  };
  for (int d = 0; d < 3; d++) {  // (as nl_create)
    h->L[d] = L[d], h->m[d] = m[d];
    const float ms_f = (float)(L[d] / m[d]);
    h->ms_f[d] = ms_f;
    h->ims_f[d] = (float)(1.0 / (double)ms_f);
    h->ims_d[d] = 1.0 / (L[d] / m[d]);
  }
  h->xy = xy, h->xz = xz, h->yz = yz;
  h->shear[0] = xy / Ly, h->shear[1] = (xz * Ly - xy * yz) / (Ly * Lz), h->shear[2] = yz / Lz;
  h->ncell = (int64_t)m[0] * m[1] * m[2];
  if (h->mesh_cells_cap > 0) {  // an initialised handle (nl_initialize, n_max 0 included): its buffers follow the mesh
    if (int rc = reserve_mesh(h, (size_t)h->n_max)) return restore(rc);
    if (!h->capacity_user) {  // estimate_capacity for the new volume, keeping the old list where it cannot grow
      const int64_t want = estimate_want(h);
      if (want > h->capacity) {
        if (int rc = swap_alloc(h, h->list, 4 * (size_t)want)) return restore(rc);
        h->capacity = want;
      }
    }
    if (int rc = stage_reserve(h)) return restore(rc);  // (the unfiltered list and the images follow the capacity)
  }
  double lat[LATTICE_CODES * 3];
  lattice_table(box_of(h), lat);
  if (hipMemcpy(h->lat_dev, lat, sizeof(lat), hipMemcpyHostToDevice) != hipSuccess) return restore(NL_ERR_HIP);
  h->upd_valid = false;
  h->built = false;
  h->t_valid = false;
  return NL_OK;
}

int nl_get_box(nl_handle_t h, double box[6]) {
  if (!h || !box) return fail(h, NL_ERR_ARG);
  box[0] = h->L[0], box[1] = h->L[1], box[2] = h->L[2], box[3] = h->xy, box[4] = h->xz, box[5] = h->yz;
  return NL_OK;
}

int nl_set_periodic(nl_handle_t h, int minimum_image) { return nl_set_periodic_axes(h, minimum_image ? 7 : 0); }

int nl_get_periodic_axes(nl_handle_t h, int* mask) {
  if (!h || !mask) return fail(h, NL_ERR_ARG);
  *mask = h->pbc;
  return NL_OK;
}

int nl_set_list_kind(nl_handle_t h, int kind) {
  if (!h || (kind != NL_LIST_HALF && kind != NL_LIST_FULL)) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  h->upd_valid = false;
  if (kind != h->list_kind) {
    h->list_kind = kind;
    h->built = false;
    h->t_valid = false;
    h->t_rows_cap = 0;  // the transposed buffer is re-allocated (and -1 filled) for the other kind
    if (h->n_max > 0)
      if (int rc = estimate_capacity(h)) return rc;
  }
  return NL_OK;
}

int nl_set_local_ids(nl_handle_t h, int on) {
  if (!h) return NL_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  h->upd_valid = false;
  if ((on != 0) != h->local_ids) {
    h->local_ids = on != 0;
    h->built = false;
    h->t_valid = false;
  }
  return NL_OK;
}

int nl_get_local_ids(nl_handle_t h, int* on) {
  if (!h || !on) return fail(h, NL_ERR_ARG);
  *on = h->local_ids ? 1 : 0;
  return NL_OK;
}

int nl_set_graph(nl_handle_t h, int on) {
  if (!h) return NL_ERR_ARG;
  h->use_graph = on != 0;
  return NL_OK;
}

int nl_set_capacity(nl_handle_t h, int64_t max_pairs) {
  if (!h || max_pairs < 0) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  h->built = false;
  h->upd_valid = false;
  int rc = dev_alloc(h, h->list, 4 * (size_t)(max_pairs + 16));
  if (rc) {
    h->capacity = 0;
    return rc;
  }
  h->capacity = max_pairs;
  h->capacity_user = true;
  return stage_reserve(h);
}

namespace {
// part = PART_ALL: the whole build.  PART_BEGIN: validate, remember the arguments, enqueue what needs only the owned
// particles.  PART_FINISH: enqueue the rest with the remembered arguments.  a: without mzl and slab, which follow from
// z_lo and z_hi.
int make_list_slab_part(nl_handle_t h, BuildArgs a, int32_t z_hi, void* stream, int sync, int part) {
  if (!h) return NL_ERR_ARG;
  if (part == PART_FINISH) {
    if (!h->begun) return fail(h, NL_ERR_STATE);
    // the second half reuses what the first half is still writing (row totals, the owned region of the sorted array):
    // it must be ordered behind it, i.e. enqueued on the same stream
    if ((hipStream_t)stream != h->last_stream) return fail(h, NL_ERR_STATE);
    a = h->args;
    z_hi = a.z_lo + a.mzl - 2 * a.slab;
  }
  h->begun = false;
  h->upd_valid = false, h->last_update = false;  // (only an update's build writes the snapshot)
  const int32_t n = a.n, n_rows = a.n_rows, z_lo = a.z_lo;
  if (h->n_max <= 0 && n > 0) return fail(h, NL_ERR_STATE);
  if (n < 0 || n_rows < 0 || n_rows > n || n > h->n_max || (a.stride != 3 && a.stride != 4) || (!a.q && n > 0))
    return fail(h, NL_ERR_ARG);
  if (a.n_ghost_lo < 0 || a.n_ghost_lo > n - n_rows) return fail(h, NL_ERR_ARG);
  if (a.gid == NL_GID_IN_W && a.stride != 4) return fail(h, NL_ERR_ARG);
  if (h->local_ids && a.gid) return fail(h, NL_ERR_ARG);  // nl_set_local_ids: the ids are the rows of q
  const int32_t mz = h->m[2];
  if (z_lo < 0 || z_hi > mz || z_lo >= z_hi) return fail(h, NL_ERR_ARG);
  const int32_t owned = z_hi - z_lo;
  a.slab = 1, a.mzl = owned + 2;
  if (owned == mz) {
    a.slab = 0, a.mzl = mz;
    if (n_rows != n) return fail(h, NL_ERR_ARG);
  } else if (mz - owned < 2) {
    return fail(h, NL_ERR_ARG);  // the two ghost layers would be the same layer
  }
  // an input-row exclusion table or a type table applies to whole single-device builds of its own particle count
  if (filter_rows_only(h) && partial_build(a, part)) return fail(h, NL_ERR_STATE);
  // nl_set_box: slab and distributed builds need the box of nl_create, and a tilt needs both of its axes periodic
  if (box_changed(h) && partial_build(a, part)) return fail(h, NL_ERR_STATE);
  if (!tilt_mask_ok(h)) return fail(h, NL_ERR_STATE);
  // nl_set_pair_images: the images are those of whole single-device builds, whose ids index the positions
  if (h->pair_images && partial_build(a, part)) return fail(h, NL_ERR_STATE);
  if (excl_refuses(h, a.gid, n_rows) || (h->ty_types && n != h->ty_n)) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = stage_reserve(h)) return rc;  // (again, if an allocation failed since a table or the flag was set)
  if (h->pending) {
    // back-to-back asynchronous builds (the reference's timing loop): errors of the previous one are dropped,
    // exactly like its results; stream order keeps the buffers consistent when the stream is the same.
    if (h->last_stream != (hipStream_t)stream) HIPCHK(h, hipStreamSynchronize(h->last_stream));
    h->pending = false;
  }
  // The build runs on exactly the stream it is given; NULL is HIP's null (default) stream, as in the reference
  // (make_list.cu:124-127 launches on the default stream), NOT a private stream: work the caller has queued on that
  // stream before the call -- e.g. the kernel that wrote the positions, or a halo exchange -- is finished first.
  hipStream_t s = (hipStream_t)stream;
  h->built = false;
  h->t_valid = false;
  h->n = n, h->n_rows = n_rows;
  // (planned before a graph key is formed: the plan's allocations bump buffers_epoch; a graph replays this plan)
  const BuildPlan p = plan_for(h, a, part, false);
  int rc;
  if (part == PART_BEGIN) {
    if ((rc = dispatch_build(h, a, p, s, nullptr, PART_BEGIN))) return rc;
    h->begun = true;
    h->last_stream = s;
    return NL_OK;
  }
  if (h->use_graph && part == PART_ALL) {
    adopt_build(h, a, p);  // (on replay: the captured build's arguments and plan, whatever ran in between)
    rc = graph_launch(h, GraphKey{a, p, h->capacity, h->buffers_epoch, h->ex_gen, h->ty_gen}, s, [&](hipStream_t cs) {
      const int rc = dispatch_build(h, a, p, cs, nullptr);
      return rc ? rc : enqueue_result_copy(h, cs);
    });
  } else {
    rc = dispatch_build(h, a, p, s, nullptr, part);
    if (!rc) rc = enqueue_result_copy(h, s);
  }
  if (rc) return rc;
  h->last_stream = s;
  h->pending = true;
  if (h->list_quiet < LIST_QUIET_BUILDS) h->list_quiet++;
  if (sync) return finish(h, true);
  return NL_OK;
}
}  // namespace

int nl_make_list_slab(nl_handle_t h, const void* q_dev, int32_t q_stride, const int32_t* gid_dev, int32_t n_rows,
                      int32_t n, int32_t z_lo, int32_t z_hi, void* stream, int sync) {
  return make_list_slab_part(h, BuildArgs{q_dev, q_stride, gid_dev, n_rows, n, 0, z_lo}, z_hi, stream, sync, PART_ALL);
}

int nl_make_list_slab_begin(nl_handle_t h, const void* q_dev, int32_t q_stride, const int32_t* gid_dev, int32_t n_rows,
                            int32_t n, int32_t n_ghost_lo, int32_t z_lo, int32_t z_hi, void* stream) {
  return make_list_slab_part(h, BuildArgs{q_dev, q_stride, gid_dev, n_rows, n, n_ghost_lo, z_lo}, z_hi, stream, 0, PART_BEGIN);
}

int nl_make_list_slab_finish(nl_handle_t h, void* stream, int sync) {
  return make_list_slab_part(h, BuildArgs{}, 0, stream, sync, PART_FINISH);
}

int nl_make_list(nl_handle_t h, const void* q_dev, int32_t q_stride, int32_t n, void* stream, int sync) {
  if (!h) return NL_ERR_ARG;
  return nl_make_list_slab(h, q_dev, q_stride, nullptr, n, n, 0, h->m[2], stream, sync);
}

int nl_synchronize(nl_handle_t h) {
  if (!h) return NL_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->pending && !h->built) return h->last_error ? h->last_error : fail(h, NL_ERR_STATE);
  return finish(h, false);
}

int nl_get_full_csr(nl_handle_t h, const int32_t** key_pointer_dev, const int32_t** list_dev,
                    const int32_t** number_of_partners_dev, int64_t* nentries) {
  return get_csr(h, true, 32, reinterpret_cast<const void**>(key_pointer_dev), list_dev, number_of_partners_dev, nentries);
}

int nl_get_half_csr(nl_handle_t h, const int32_t** key_pointer_dev, const int32_t** sorted_list_dev,
                    const int32_t** number_of_partners_dev, int64_t* npairs) {
  return get_csr(h, false, 32, reinterpret_cast<const void**>(key_pointer_dev), sorted_list_dev, number_of_partners_dev, npairs);
}

int nl_get_full_csr64(nl_handle_t h, const int64_t** key_pointer_dev, const int32_t** list_dev,
                      const int32_t** number_of_partners_dev, int64_t* nentries) {
  return get_csr(h, true, 64, reinterpret_cast<const void**>(key_pointer_dev), list_dev, number_of_partners_dev, nentries);
}

int nl_get_half_csr64(nl_handle_t h, const int64_t** key_pointer_dev, const int32_t** sorted_list_dev,
                      const int32_t** number_of_partners_dev, int64_t* npairs) {
  return get_csr(h, false, 64, reinterpret_cast<const void**>(key_pointer_dev), sorted_list_dev, number_of_partners_dev, npairs);
}

int nl_list_checksum(nl_handle_t h, uint64_t* checksum, int64_t* nentries) {
  if (!h || !checksum) return fail(h, NL_ERR_ARG);
  int rc = nl_synchronize(h);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->last_stream;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(h->totals + 3);
  HIPCHK(h, hipMemsetAsync(acc, 0, 8, s));
  const int32_t n = h->n_rows;
  if (n > 0) {
    const int32_t grid = std::max(1, std::min((n + 3) / 4, 8 * h->num_cus));
    const bool w = h->plan.wide, f32 = h->dtype == NL_F32;
    const int32_t* gid = h->args.gid;
    const void* q = h->args.q;
    if (f32 && !w)
      hipLaunchKernelGGL((k_list_checksum<float, int32_t>), dim3(grid), dim3(256), 0, s, static_cast<const int32_t*>(h->key_pointer), h->list, n, gid, static_cast<const float*>(q), acc);
    else if (f32)
      hipLaunchKernelGGL((k_list_checksum<float, int64_t>), dim3(grid), dim3(256), 0, s, static_cast<const int64_t*>(h->key_pointer), h->list, n, gid, static_cast<const float*>(q), acc);
    else if (!w)
      hipLaunchKernelGGL((k_list_checksum<double, int32_t>), dim3(grid), dim3(256), 0, s, static_cast<const int32_t*>(h->key_pointer), h->list, n, gid, static_cast<const double*>(q), acc);
    else
      hipLaunchKernelGGL((k_list_checksum<double, int64_t>), dim3(grid), dim3(256), 0, s, static_cast<const int64_t*>(h->key_pointer), h->list, n, gid, static_cast<const double*>(q), acc);
    HIPCHK(h, hipGetLastError());
  }
  unsigned long long out = 0;
  HIPCHK(h, hipMemcpyAsync(&out, acc, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  *checksum = (uint64_t)out;
  if (nentries) *nentries = list_total(h);
  return NL_OK;
}

int nl_get_cell_order(nl_handle_t h, const int32_t** order_dev, int32_t* n) {
  if (!h) return NL_ERR_ARG;
  int rc = nl_synchronize(h);
  if (rc) return rc;
  if (order_dev) *order_dev = h->sorted_row;
  if (n) *n = h->n;
  return NL_OK;
}

int nl_resort(nl_handle_t h, void* array_dev, size_t elem_bytes, void* stream) {
  if (!h || !array_dev || elem_bytes == 0 || elem_bytes % 4 != 0 || elem_bytes > 32 || elem_bytes == 20 || elem_bytes == 28)
    return fail(h, NL_ERR_ARG);
  int rc = nl_synchronize(h);  // the permutation is the last build's
  if (rc) return rc;
  if (h->args.slab || h->n_rows != h->n) return fail(h, NL_ERR_STATE);  // a permutation of the caller's own particles
  h->upd_valid = false;  // (the snapshot holds the old order)
  HIPCHK(h, hipSetDevice(h->device));
  const int32_t n = h->n;
  if (n == 0) return NL_OK;
  if (h->ex_relabel) {  // the first re-sort after a build: the tables follow the particles, once
    if (h->ex_ids && !h->ex_global && h->ex_n == n)  // (a global table's ids are the caller's names, not rows)
      if ((rc = excl_relabel(h))) return rc;
    if (h->ty_types && h->ty_n == n)
      if ((rc = types_relabel(h))) return rc;
    h->ex_relabel = false;
  }
  if (!h->resort_buf)
    if ((rc = side_alloc(h, h->resort_buf, 32 * ((size_t)h->n_max + 16)))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (s != h->last_stream) HIPCHK(h, hipStreamSynchronize(h->last_stream));
  const uint32_t* src = static_cast<const uint32_t*>(array_dev);
  uint32_t* buf = static_cast<uint32_t*>(h->resort_buf);
  const dim3 grid((n + 255) / 256), block(256);
  switch (elem_bytes / 4) {
    case 1: hipLaunchKernelGGL(k_gather_words<1>, grid, block, 0, s, src, h->sorted_row, n, buf); break;
    case 2: hipLaunchKernelGGL(k_gather_words<2>, grid, block, 0, s, src, h->sorted_row, n, buf); break;
    case 3: hipLaunchKernelGGL(k_gather_words<3>, grid, block, 0, s, src, h->sorted_row, n, buf); break;
    case 4: hipLaunchKernelGGL(k_gather_words<4>, grid, block, 0, s, src, h->sorted_row, n, buf); break;
    case 6: hipLaunchKernelGGL(k_gather_words<6>, grid, block, 0, s, src, h->sorted_row, n, buf); break;
    default: hipLaunchKernelGGL(k_gather_words<8>, grid, block, 0, s, src, h->sorted_row, n, buf); break;
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(array_dev, buf, elem_bytes * (size_t)n, hipMemcpyDeviceToDevice, s));
  return NL_OK;
}

int nl_set_offset_width(nl_handle_t h, int bits) {
  if (!h || (bits != 0 && bits != 32 && bits != 64)) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  h->upd_valid = false;
  if (bits != h->offset_width) {
    h->offset_width = bits;
    h->built = false;
    h->t_valid = false;
  }
  return NL_OK;
}

int nl_number_of_pairs(nl_handle_t h, int64_t* npairs) {
  if (!h || !npairs) return fail(h, NL_ERR_ARG);
  int rc = nl_synchronize(h);
  if (rc) return rc;
  *npairs = h->plan.full ? list_total(h) / 2 : list_total(h);
  return NL_OK;
}

int nl_get_mesh(nl_handle_t h, int32_t mesh[3], int64_t* ncell) {
  if (!h) return NL_ERR_ARG;
  if (mesh)
    for (int d = 0; d < 3; d++) mesh[d] = h->m[d];
  if (ncell) *ncell = h->ncell;
  return NL_OK;
}

int nl_get_sorted(nl_handle_t h, const int32_t** cell_start_dev, const void** sorted_pos_dev,
                  const int32_t** sorted_row_dev, int64_t* ncell_local) {
  if (!h) return NL_ERR_ARG;
  int rc = nl_synchronize(h);
  if (rc) return rc;
  if (cell_start_dev) *cell_start_dev = h->cell_start;
  if (sorted_pos_dev) *sorted_pos_dev = h->sorted;
  if (sorted_row_dev) *sorted_row_dev = h->sorted_row;
  if (ncell_local) *ncell_local = (int64_t)h->m[0] * h->m[1] * h->args.mzl;
  return NL_OK;
}

int nl_debug_read(nl_handle_t h, uint64_t* out, int32_t n, int reset) {
  if (!h || !out || !h->dbg_buf || n < 0 || n > 64 + 4 * 4096) return NL_ERR_ARG;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(out, h->dbg_buf, 8 * (size_t)n, hipMemcpyDeviceToHost));
  if (reset) HIPCHK(h, hipMemset(h->dbg_buf, 0, 8 * (64 + 4 * 4096)));
  return NL_OK;
}

int nl_debug_occupancy(int32_t out[8]) {
  if (!out) return NL_ERR_ARG;
  int v = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return NL_ERR_NO_DEVICE;
  out[0] = (int32_t)(prop.maxSharedMemoryPerMultiProcessor / 1024);
  out[1] = (int32_t)(prop.sharedMemPerBlock / 1024);
  out[2] = out[3] = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_sweep_count_f32<false, false>, SWEEP_WAVES * WAVE, 0);
  out[4] = v;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_sweep<float, MODE_FILL>, SWEEP_WAVES * WAVE, 0);
  out[5] = v;
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_sweep_count_masks_f32<false, false>));
  out[6] = (int32_t)fa.sharedSizeBytes;
  out[7] = fa.numRegs;
  return NL_OK;
}

int nl_get_build_info(nl_handle_t h, int32_t info[8]) {
  if (!h || !info) return NL_ERR_ARG;
  for (int k = 4; k < 8; k++) info[k] = 0;
  const BuildPlan& p = h->plan;
  info[4] = p.wide ? 64 : 32;
  info[5] = p.mask_nb;
  info[6] = p.search == SEARCH_ROWS ? 1 + p.rows_v : 0;  // fine-row search: the cell table of nl_get_sorted is the fine-row table
  // (bits 8..15: classes of an id-class build; bits 16..17: the binning, 0 = two-pass, 1 = bucket, 2 = atomic rank;
  // bit 18: the reach cull)
  const int32_t binning = p.binning == BINNING_TWO_PASS ? 0 : p.binning == BINNING_BUCKET ? 1 : 2;
  info[7] = (p.small ? 1 : 0) | p.idc << 8 | binning << 16 | (p.cull ? 1 : 0) << 18;
  info[0] = p.search != SEARCH_SWEEPS ? 1 : 0;
  info[1] = h->sweep_variant;
  info[2] = h->dtype == NL_F32 ? SweepCfg<float>::CAP : SweepCfg<double>::CAP;
  info[3] = h->num_cus;
  return NL_OK;
}

int nl_get_build_stats(nl_handle_t h, int64_t stats[4]) {
  if (!h || !stats) return NL_ERR_ARG;
  stats[0] = h->reruns[0];
  stats[1] = h->reruns[1];
  stats[2] = h->plan.cap_row;
  stats[3] = h->plan.list ? 1 : 0;
  return NL_OK;
}

int nl_last_error(nl_handle_t h) { return h ? h->last_error : NL_ERR_ARG; }
int nl_last_hip_error(nl_handle_t h) { return h ? h->last_hip : 0; }

int nl_profile_last_build(nl_handle_t h, int32_t reps, double ms[NL_NUM_STAGES]) {
  if (!h || !ms || reps <= 0) return fail(h, NL_ERR_ARG);
  int rc = nl_synchronize(h);  // the build being profiled must have succeeded (buffers sized, list large enough)
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  for (int k = 0; k < NL_NUM_STAGES; k++) ms[k] = 0;
  hipStream_t s = h->own_stream;
  HIPCHK(h, hipStreamSynchronize(h->last_stream));
  BuildArgs a = h->args;
  a.n = h->n;  // (a distributed build: the particles finish() has counted)
  // the builds below replace the list with one of the positions as they are now: not an update's build, and the snapshot
  // is no longer the list's (as nl_make_list); nor is a transposed list made before them
  h->upd_valid = false, h->last_update = false;
  h->built = false;
  h->t_valid = false;
  // one whole build, planned as the last one was: with the two-pass binning and every launch where finish() had run
  // it again or an update had built it, so that build_info() keeps describing the build the caller made
  const BuildPlan p = plan_for(h, a, PART_ALL, h->plan.rerun);
  for (int r = 0; r < reps; r++) {
    rc = dispatch_build(h, a, p, s, h->ev);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    for (int k = 0; k < NL_STAGE_TOTAL; k++) {
      float t = 0;
      HIPCHK(h, hipEventElapsedTime(&t, h->ev[k], h->ev[k + 1]));
      ms[k] += t;
    }
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, h->ev[0], h->ev[NL_STAGE_TOTAL]));
    ms[NL_STAGE_TOTAL] += t;
  }
  for (int k = 0; k < NL_NUM_STAGES; k++) ms[k] /= reps;
  rc = enqueue_result_copy(h, s);
  if (rc) return rc;
  h->last_stream = s;
  h->pending = true;
  return finish(h, false);
}

int nl_profile_stages(nl_handle_t h, const void* q_dev, int32_t q_stride, int32_t n, int32_t reps,
                      double ms[NL_NUM_STAGES]) {
  if (!h || !ms || reps <= 0) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());  // diagnostic entry point: whatever produced q, on whichever stream, is done
  int rc = nl_make_list(h, q_dev, q_stride, n, nullptr, 1);
  if (rc) return rc;
  return nl_profile_last_build(h, reps, ms);
}

/* ------------------------------------------------------------------ buffers */

int nl_buf_alloc(void** dev, void** host, size_t bytes) {
  if (!dev && !host) return NL_ERR_ARG;
  if (dev) *dev = nullptr;
  if (host) *host = nullptr;
  if (dev && hipMalloc(dev, bytes ? bytes : 16) != hipSuccess) return NL_ERR_NOMEM;
  if (host && hipHostMalloc(host, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
    if (dev) {
      (void)hipFree(*dev);
      *dev = nullptr;
    }
    return NL_ERR_NOMEM;
  }
  return NL_OK;
}
int nl_buf_free(void* dev, void* host) {
  int rc = NL_OK;
  if (dev && hipFree(dev) != hipSuccess) rc = NL_ERR_HIP;
  if (host && hipHostFree(host) != hipSuccess) rc = NL_ERR_HIP;
  return rc;
}
int nl_buf_h2d(void* dev, const void* host, size_t bytes) {
  return hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) == hipSuccess ? NL_OK : NL_ERR_HIP;
}
int nl_buf_d2h(void* host, const void* dev, size_t bytes) {
  return hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess ? NL_OK : NL_ERR_HIP;
}
int nl_buf_fill32(void* dev, uint32_t pattern, size_t count) {
  if (hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(dev), (int)pattern, count) != hipSuccess) return NL_ERR_HIP;
  return hipDeviceSynchronize() == hipSuccess ? NL_OK : NL_ERR_HIP;
}
int nl_buf_fill64(void* dev, uint64_t pattern, size_t count) {
  // two interleaved 32-bit patterns: fill as 32-bit words when both halves agree, else through a staging copy
  const uint32_t lo = (uint32_t)pattern, hi = (uint32_t)(pattern >> 32);
  if (lo == hi) return nl_buf_fill32(dev, lo, count * 2);
  uint64_t* tmp = static_cast<uint64_t*>(malloc(sizeof(uint64_t) * (count ? count : 1)));
  if (!tmp) return NL_ERR_NOMEM;
  for (size_t i = 0; i < count; i++) tmp[i] = pattern;
  const hipError_t e = hipMemcpy(dev, tmp, sizeof(uint64_t) * count, hipMemcpyHostToDevice);
  free(tmp);
  return e == hipSuccess ? NL_OK : NL_ERR_HIP;
}
int nl_device_synchronize(void) { return hipDeviceSynchronize() == hipSuccess ? NL_OK : NL_ERR_HIP; }

}  // extern "C"

#include "nl_transpose.inc"
#include "nl_skin.inc"
#include "nl_consumer.inc"
#include "nl_dist.inc"
#include "nl_exclude.inc"
#include "nl_types.inc"
#include "nl_images.inc"
#include "nl_virial.inc"
#include "nl_table.inc"
#include "nl_eam.inc"
#include "nl_sw.inc"
#include "nl_tersoff.inc"
#include "nl_coulomb.inc"
#include "nl_coul_excl.inc"
#include "nl_dpd.inc"
#include "nl_histogram.inc"
#include "nl_steinhardt.inc"
#include "nl_cluster.inc"
#include "nl_cna.inc"
