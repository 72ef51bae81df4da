// nl_cluster.inc -- clusters from the list of the last build (DESIGN.md section 8za): the connected components of the graph
// whose edges are the stored pairs within r_max between members (nl_clusters), and the ten Wolde-Frenkel count of solid-like
// bonds per particle from the q_lm of the last nl_steinhardt call (nl_solid_bonds).  The rules are stated at nl_clusters in
// include/nl_hip.h.  The first consumer whose rows depend on each other across the whole grid: a lock-free union-find
// (nl_unionfind.hpp) on the caller's own label array,
//   k_cc_init      parent[i] = i, the counters and the summary zeroed;
//   k_cc_union     one wave per row over lj_row_pairs (the histogram's walk, LjScalars "none"), unite(row, j) for every edge;
//   k_cc_flatten   labels[i] = the root of i, or -1 for a non-member; count[root] += 1;
//   k_cc_sizes     sizes[i] = count[labels[i]]; members, clusters and the largest cluster by integer atomics;
//   k_cc_summary   one thread unpacks the largest cluster's {size, label}.
// labels_dev is the parent array and sizes_dev the counter array: no scratch, but for the counters of a call that asks for the
// summary without the sizes (cc_part, first_call_scratch).  Integers only: the answer is exact and the same bytes for every
// schedule, build and list kind.
// The pieces are those of nl_consumer.inc (LjArgs, lj_args, lj_row_pairs, grid_rows, consumer_call, list_reach, first_call_scratch),
// hist_edge and hist_reach of nl_histogram.inc, stein_reach and the q_lm scratch of nl_steinhardt.inc and sqrt_t of nl_sw.inc.
// Included at the end of nl_api.hip, behind nl_steinhardt.inc.

#include "nl_unionfind.hpp"

namespace {

constexpr int CC_BLOCKS = 2048;  // the most blocks of every kernel here (the grid of k_pair_hist)
constexpr unsigned long long CC_LABEL_TOP = 0x7fffffffull;  // the packed largest cluster: (size << 32) | (CC_LABEL_TOP - label)

// What a launch needs beside LjArgs.  count: sizes_dev, or the scratch where the caller wants the summary alone, or nullptr
// where it wants neither.
struct CcArgs {
  double r_max;
  int32_t full, min_member;
  const int32_t* __restrict__ member;  // nullptr: everybody
  int32_t* parent;                     // labels_dev
  int32_t* count;
  int32_t* sizes;                      // sizes_dev or nullptr
  unsigned long long* summary;         // summary_dev or nullptr
};

__device__ __forceinline__ bool cc_member(const CcArgs& g, int32_t i) { return !g.member || g.member[i] >= g.min_member; }

// The rows of a grid of one thread per particle.
template <typename F> __device__ __forceinline__ void cc_particles(int32_t n, F&& f) {
  for (int32_t i = (int32_t)blockIdx.x * STAGE_THREADS + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * STAGE_THREADS) f(i);
}

// parent[i] = i; counters and summary zeroed.  A failed list (status, the enqueue variant): the fills of the contract, and the
// kernels behind this one do nothing.
__global__ void __launch_bounds__(STAGE_THREADS) k_cc_init(int32_t n, const uint32_t* __restrict__ status, CcArgs g) {
  const bool dead = status && *status != 0u;  // (uniform over the launch)
  cc_particles(n, [&](int32_t i) {
    g.parent[i] = dead ? -1 : i;
    if (g.count) g.count[i] = 0;
  });
  if (g.summary && blockIdx.x == 0 && threadIdx.x < 4) g.summary[threadIdx.x] = dead ? ~0ull : 0ull;
}

// One wave per row, the rows dealt to the waves of the grid in turn (k_pair_hist's).  An entry is an edge iff both ends are
// members and r2 < X; after a full build only the entries with j > row are used, so both list kinds unite the same pairs.
// Every access to the parent array in this kernel is an agent-scope atomic (UfDevice): the array is written by other CUs while
// this one reads it, a CU's L1 is never refreshed by their stores and the XCDs' L2s are not coherent for plain stores, so a
// plain load could return a line cached before the kernel wrote it and a plain store could stay in one XCD's L2.  (k_cc_init's
// plain stores are behind a kernel boundary.)  No fence: nothing here depends on the order of two accesses.
// No thread waits for another: uf_unite ends by its own progress (nl_unionfind.hpp), and the dependence between the kernels
// is the stream's.
template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_cc_union(LjArgs<T, OFF> a, CcArgs g) {
  if (a.status && *a.status != 0u) return;  // (uniform over the launch) a failed list is not read
  const T X = hist_edge<T>(1, g.r_max, 1);
  const LjScalars<T> none = {(T)0, (T)0, (T)0};
  grid_rows(a.n, [&](int32_t row, int32_t lane) {
    if (!cc_member(g, row)) return;  // (uniform over the wave)
    lj_row_pairs<T, OFF, TRI>(a, none, row, lane, [&](int32_t j, LjPartner, T dx, T dy, T dz, T, T, T, T, bool) {
      if (g.full && j <= row) return;  // a pair stored twice is united once, from the row of the smaller id
      const T r2 = (dx * dx + dy * dy) + dz * dz;
      if (!(r2 < X)) return;  // beyond r_max, or NaN
      if (!cc_member(g, j)) return;
      nl::uf_unite<nl::UfDevice>(g.parent, row, j);
    });
  });
}

// labels[i] = the root of i (no union runs any more: the roots are final, and minimum-hooking made each the smallest index of
// its component), -1 for a non-member; count[root] += 1, an integer add.  The stores go to the array other threads of this
// kernel still walk, so they are atomics like the loads (k_cc_union's reason): a member's new parent is its root, a vertex of
// its tree below it, and a non-member is a tree of its own that nobody else's walk enters.  The walk is uf_root, which stores
// nothing: every entry is written by its own thread alone, once, so what it wrote is the label (a halving store of another
// thread's walk, arriving late, would put an older ancestor back over it).
__global__ void __launch_bounds__(STAGE_THREADS) k_cc_flatten(int32_t n, const uint32_t* __restrict__ status, CcArgs g) {
  if (status && *status != 0u) return;
  cc_particles(n, [&](int32_t i) {
    if (!cc_member(g, i)) {
      nl::UfDevice::store(g.parent + i, -1);
      return;
    }
    const int32_t r = nl::uf_root<nl::UfDevice>(g.parent, i);
    if (r != i) nl::UfDevice::store(g.parent + i, r);
    if (g.count) atomicAdd(&g.count[r], 1);
  });
}

// sizes[i] = count[labels[i]].  In place where count is sizes: a root's entry already holds its size and is only read, every
// other particle writes its own entry, which nobody reads.  The summary: one add per block to members and clusters, one 64-bit
// max per block of (size << 32) | (CC_LABEL_TOP - label) over the roots -- the larger size wins and among equals the smaller
// label.  Plain loads: everything read was written by the kernels before.
__global__ void __launch_bounds__(STAGE_THREADS) k_cc_sizes(int32_t n, const uint32_t* __restrict__ status, CcArgs g) {
  if (status && *status != 0u) return;
  __shared__ unsigned long long blk[3];
  if (threadIdx.x < 3) blk[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t members = 0, roots = 0;  // (of this thread, then of its wave: below n)
  unsigned long long best = 0;
  cc_particles(n, [&](int32_t i) {
    const int32_t lab = g.parent[i];
    const int32_t sz = lab >= 0 ? g.count[lab] : 0;
    if (g.sizes && lab != i) g.sizes[i] = sz;
    if (lab >= 0) members++;
    if (lab == i) roots++, best = max(best, ((unsigned long long)(uint32_t)sz << 32) | (CC_LABEL_TOP - (unsigned long long)lab));
  });
  if (!g.summary) return;  // (uniform)
  members = wave_sum(members), roots = wave_sum(roots);
  if ((threadIdx.x & 63) == 0 && members) atomicAdd(&blk[0], (unsigned long long)members), atomicAdd(&blk[1], (unsigned long long)roots);
  if (best) atomicMax(&blk[2], best);
  __syncthreads();
  if (threadIdx.x == 0 && blk[0]) {
    atomicAdd(&g.summary[0], blk[0]);
    if (blk[1]) atomicAdd(&g.summary[1], blk[1]), atomicMax(&g.summary[2], blk[2]);
  }
}

// {size, label} of the largest cluster from the packed word; no member: {0, -1}.
__global__ void k_cc_summary(const uint32_t* __restrict__ status, unsigned long long* summary) {
  if (status && *status != 0u) return;
  const unsigned long long p = summary[2];
  const unsigned long long size = p >> 32;
  summary[2] = size;
  summary[3] = size ? CC_LABEL_TOP - (p & 0xffffffffull) : ~0ull;
}

// ---- the solid-bond count
template <typename T> struct SolidArgs {
  int32_t l;
  double r_max;
  T thr;
  const T* __restrict__ qlm;  // [n][l + 1][2] of the last nl_steinhardt call
  int32_t* __restrict__ count;
};

// D of two q_lm rows: (re_0 re'_0 + im_0 im'_0) + 2 sum_{m = 1 .. l} (re_m re'_m + im_m im'_m), m ascending; 2 S is S + S.
template <typename T>
__device__ __forceinline__ T solid_dot(const T (&ar)[STEIN_M], const T (&ai)[STEIN_M], const T (&br)[STEIN_M], const T (&bi)[STEIN_M], int32_t l) {
  T s = (T)0;
#pragma unroll
  for (int m = 1; m < STEIN_M; m++) {
    if (m <= l) s += ar[m] * br[m] + ai[m] * bi[m];  // (uniform)
  }
  return (ar[0] * br[0] + ai[0] * bi[0]) + (s + s);
}

// One wave per row.  Every lane keeps the row's q_lm in registers (the unrolled m loop of k_stein_out's second walk); a lane
// whose entry is a neighbour gathers the partner's 2 (l + 1) values once, forms D_ij and s_j from them and tests
// D_ij > thr sqrt(s_i s_j) -- false for a NaN on either side.  One wave_sum of the lanes' counts per row; no atomic.
template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_solid_bonds(LjArgs<T, OFF> a, SolidArgs<T> g) {
  const int32_t l = g.l, nm = l + 1;
  const T X = hist_edge<T>(1, g.r_max, 1);
  const LjScalars<T> none = {(T)0, (T)0, (T)0};
  const bool dead = a.status && *a.status != 0u;  // (uniform over the launch)
  grid_rows(a.n, [&](int32_t row, int32_t lane) {
    if (dead) {
      if (lane == 0) g.count[row] = -1;
      return;
    }
    T ir[STEIN_M], ii[STEIN_M];
    const T* qi = g.qlm + (size_t)row * nm * 2;
#pragma unroll
    for (int m = 0; m < STEIN_M; m++) {
      ir[m] = ii[m] = (T)0;
      if (m <= l) ir[m] = qi[2 * m], ii[m] = qi[2 * m + 1];  // (uniform)
    }
    const T si = solid_dot(ir, ii, ir, ii, l);
    int32_t cnt = 0;
    lj_row_pairs<T, OFF, TRI>(a, none, row, lane, [&](int32_t j, LjPartner, T dx, T dy, T dz, T, T, T, T, bool) {
      const T r2 = (dx * dx + dy * dy) + dz * dz;
      if (!(r2 < X && r2 > (T)0)) return;
      T jr[STEIN_M], ji[STEIN_M];
      const T* qj = g.qlm + (size_t)j * nm * 2;
#pragma unroll
      for (int m = 0; m < STEIN_M; m++) {
        jr[m] = ji[m] = (T)0;
        if (m <= l) jr[m] = qj[2 * m], ji[m] = qj[2 * m + 1];  // (uniform)
      }
      const T d = solid_dot(ir, ii, jr, ji, l), sj = solid_dot(jr, ji, jr, ji, l);
      if (d > g.thr * sqrt_t(si * sj)) cnt++;
    });
    cnt = wave_sum(cnt);
    if (lane == 0) g.count[row] = cnt;
  });
}

// ---- host side
// The counters of a call that wants the summary without the sizes: int32 [n_max + 16], by Steinhardt's rule -- the first call
// that needs it allocates (NL_ERR_STATE inside a capture), and again after an nl_initialize with another n_max.
int cc_scratch(nl_handle_t h, hipStream_t s) {
  if (h->cc_part && h->cc_cap_n != h->n_max) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(h, hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(h, NL_ERR_STATE);
    HIPCHK(h, hipDeviceSynchronize());  // (a call in flight may still write the old one)
    h->cc_part.release();
  }
  if (h->cc_part) return NL_OK;
  if (int rc = first_call_scratch(h, h->cc_part, 4 * ((size_t)h->n_max + 16), s)) return rc;
  h->cc_cap_n = h->n_max;
  return NL_OK;
}

int cc_launch(nl_handle_t h, const void* q_dev, int32_t stride, double r_max, const int32_t* member_dev, int32_t min_member,
              int32_t* labels_dev, int32_t* sizes_dev, int64_t* summary_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  int32_t* count = sizes_dev;
  if (!count && summary_dev) {
    if (int rc = cc_scratch(h, s)) return rc;
    count = h->cc_part.get();
  }
  const CcArgs g = {r_max, h->plan.full ? 1 : 0, min_member, member_dev, labels_dev, count, sizes_dev,
                    reinterpret_cast<unsigned long long*>(summary_dev)};
  const int32_t nthr = (int32_t)std::min<int64_t>(((int64_t)n + STAGE_THREADS - 1) / STAGE_THREADS, CC_BLOCKS);
  const int32_t nrow = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, CC_BLOCKS);
  hipLaunchKernelGGL(k_cc_init, dim3(nthr), dim3(STAGE_THREADS), 0, s, n, status, g);
  const int rc = dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    with_flag(h->plan.tilt, [&](auto tri) {
      hipLaunchKernelGGL((k_cc_union<T, OFF, decltype(tri)::value>), dim3(nrow), dim3(STAGE_THREADS), 0, s, a, g);
    });
    return NL_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_cc_flatten, dim3(nthr), dim3(STAGE_THREADS), 0, s, n, status, g);
  if (count) hipLaunchKernelGGL(k_cc_sizes, dim3(nthr), dim3(STAGE_THREADS), 0, s, n, status, g);
  if (summary_dev) hipLaunchKernelGGL(k_cc_summary, dim3(1), dim3(1), 0, s, status, g.summary);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

// A whole single-device list, half or full (a cluster spans ranks: slab and distributed builds are refused, local-index ones
// included, which consumer_ready lets through); then the untyped histogram's reach.
int cc_reach(nl_handle_t h, double r_max, double skin) {
  if (h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  return hist_reach(h, r_max, false, skin);
}

int cc_call(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, const int32_t* member_dev, int32_t min_member,
            int32_t* labels_dev, int32_t* sizes_dev, int64_t* summary_dev, void* stream, bool enqueue) {
  return consumer_call(
      h, q_dev, q_stride, labels_dev, r_max > 0 && std::isfinite(r_max), stream, enqueue,
      [&](double skin) { return cc_reach(h, r_max, skin); },
      [&](hipStream_t s, const uint32_t* status) {
        return cc_launch(h, q_dev, q_stride, r_max, member_dev, min_member, labels_dev, sizes_dev, summary_dev, s, status);
      });
}

int solid_launch(nl_handle_t h, const void* q_dev, int32_t stride, double threshold, int32_t* count_dev, hipStream_t s,
                 const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, STEIN_BLOCKS);
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    const SolidArgs<T> g = {h->st_last_l, h->st_rmax, (T)threshold, static_cast<const T*>(h->st_part.get()), count_dev};
    with_flag(h->plan.tilt, [&](auto tri) {
      hipLaunchKernelGGL((k_solid_bonds<T, OFF, decltype(tri)::value>), dim3(nblk), dim3(STAGE_THREADS), 0, s, a, g);
    });
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

// Steinhardt's lists and reach, and the q_lm of a call (the condition of nl_steinhardt_get_qlm).
int solid_reach(nl_handle_t h, double skin) {
  if (int rc = stein_reach(h, skin)) return rc;
  if (!h->st_part || h->st_last_l == 0 || h->st_cap_n != h->n_max) return fail(h, NL_ERR_STATE);
  return NL_OK;
}

int solid_call(nl_handle_t h, const void* q_dev, int32_t q_stride, double threshold, int32_t* count_dev, void* stream, bool enqueue) {
  return consumer_call(
      h, q_dev, q_stride, count_dev, threshold > -1.0 && threshold < 1.0, stream, enqueue,
      [&](double skin) { return solid_reach(h, skin); },
      [&](hipStream_t s, const uint32_t* status) { return solid_launch(h, q_dev, q_stride, threshold, count_dev, s, status); });
}

}  // namespace

extern "C" {

int nl_clusters(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, const int32_t* member_dev, int32_t min_member,
                int32_t* labels_dev, int32_t* sizes_dev, int64_t* summary_dev, void* stream) {
  return cc_call(h, q_dev, q_stride, r_max, member_dev, min_member, labels_dev, sizes_dev, summary_dev, stream, false);
}
int nl_clusters_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, const int32_t* member_dev,
                        int32_t min_member, int32_t* labels_dev, int32_t* sizes_dev, int64_t* summary_dev, void* stream) {
  return cc_call(h, q_dev, q_stride, r_max, member_dev, min_member, labels_dev, sizes_dev, summary_dev, stream, true);
}
int nl_solid_bonds(nl_handle_t h, const void* q_dev, int32_t q_stride, double threshold, int32_t* count_dev, void* stream) {
  return solid_call(h, q_dev, q_stride, threshold, count_dev, stream, false);
}
int nl_solid_bonds_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double threshold, int32_t* count_dev, void* stream) {
  return solid_call(h, q_dev, q_stride, threshold, count_dev, stream, true);
}

}  // extern "C"
