// nl_table.inc -- tabulated pair potentials (DESIGN.md section 8o): forces, per-particle energies and the totals of
// nl_virial.inc for any pair potential the caller has sampled (nl_set_pair_table), from the list of the last build.  The rule
// is stated at nl_set_pair_table in include/nl_hip.h.  A second pair function on the walk of section 8l: TableByPair is the
// PAR of lj_row_at and lj_virial_rows, and the launches and entry points are the shared ones of nl_consumer.inc and
// nl_virial.inc (rows_launch, totals_launch, pair_call) with the table's own reach.
// What a table is, is written once, here, for this file and nl_eam.inc (DESIGN.md section 8q): a table as a kernel sees it
// (TableView: its knot of r^2, a particle's type, a slot), its staging into LDS (table_stage), and on the host the handle's
// TableSet, its view (table_view), its reach (table_set_reach) and its upload (table_upload).
// The grid of the forces: k_lj takes one block per 4 rows, which a block that first stages a table of 16 KiB cannot afford, so
// k_table_forces is persistent -- at most NL_TABLE_BLOCKS blocks, each stages the table once and its waves then walk
// grid_rows (k_table_virial: the grid lj_virial_rows has always had).
// A table larger than NL_TABLE_LDS_BYTES (or one set under NL_TABLE_LDS=0) is read from global memory instead: the same
// knots, the same arithmetic, the same bits.
// Included at the end of nl_api.hip, behind nl_virial.inc.

namespace {

static_assert(NL_TABLE_BLOCKS <= VIR_BLOCKS, "k_table_virial leaves its partials in vir_part");
static_assert(NL_TABLE_LDS_BYTES + sizeof(double) * 4 * VIR_OUT <= 65536, "the table and the block partials of k_table_virial in 64 KiB of LDS");

// One knot of one slot: the value at x_k and the difference to the next knot (0 at the last), in the position type.
// 16 bytes in fp32: one ds_read_b128 / global_load_dwordx4 per entry; two in fp64.
template <typename T> struct alignas(16) TableKnot {
  T F, dF, U, dU;
};

// The knot of r2 on a grid uniform in r^2 (linear in r^2 between the knots: no square root, one knot read).  in: within r_max,
// and not the particle itself; below: under r_min, where a table has no value; k, t: the knot and the place behind it (s >= 0
// where k is taken; outside, knot 0 is read and dropped).  A value v + t dv is read as in ? (below ? NaN : v + t dv) : 0.
template <typename T> struct TableAt {
  bool in, below;
  int32_t k;
  T t;
};
template <typename T> __device__ __forceinline__ TableAt<T> table_knot(T r2, T x0, T xc, T iD, int32_t nknots) {
  const bool in = r2 < xc && r2 > (T)0;
  const T s = (r2 - x0) * iD;
  const bool below = r2 < x0;
  const int32_t k = in && !below ? min((int32_t)s, nknots - 2) : 0;
  return {in, below, k, s - (T)k};
}

// A table as a kernel sees it.
template <typename T> struct TableView {
  const TableKnot<T>* tab;  // [nslots][nknots], in LDS or in global memory
  T x0, xc, iD;             // r_min^2, r_max^2, 1 / D
  int32_t nknots, ntypes;
  const int32_t* __restrict__ types;  // ntypes > 1: the handle's type table; else nullptr
  __device__ __forceinline__ TableAt<T> knot(T r2) const { return table_knot(r2, x0, xc, iD, nknots); }
  __device__ __forceinline__ int32_t type(int32_t i) const { return type_of(types, i, ntypes); }
  // a table with a slot per type, and one with a slot per unordered pair of types
  __device__ __forceinline__ const TableKnot<T>* slot(int32_t t) const { return tab + (size_t)t * nknots; }
  __device__ __forceinline__ const TableKnot<T>* slot(int32_t ti, int32_t j) const {
    if (!types) return tab;
    return slot(pair_slot(ti, type(j), ntypes));
  }
};

template <typename T> struct TableByPair {
  static constexpr bool lanes_meet = false, table = true;  // (every lane reads its own knot: nothing to exchange)
  TableView<T> v;
  __device__ __forceinline__ int32_t row(int32_t row, int32_t) const { return v.type(row); }
  __device__ __forceinline__ const TableKnot<T>* entry(int32_t ti, int32_t j) const { return v.slot(ti, j); }
  // table_knot and the two reads, spelled out: behind any function (v.knot, a by-reference form, a member that reads the
  // view's fields) the 48 instances take other registers than their parents (section 8q), so the text stays here.
  __device__ __forceinline__ void pair(const TableKnot<T>* slot, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    in = r2 < v.xc && r2 > (T)0;
    const T s = (r2 - v.x0) * v.iD;
    const bool below = r2 < v.x0;
    const int32_t k = in && !below ? min((int32_t)s, v.nknots - 2) : 0;
    const TableKnot<T> w = slot[k];
    const T t = s - (T)k;
    const T fr = in ? (below ? (T)NAN : w.F + t * w.dF) : (T)0;
    pe = in ? (below ? (T)NAN : w.U + t * w.dU) : (T)0;
    fx = fr * dx, fy = fr * dy, fz = fr * dz;
  }
};

// One table, or two one after the other, into the block's dynamic LDS, 16 bytes per thread and step; the views then read
// there.  na16, nb16: the tables in 16-byte words.
template <typename T>
__device__ __forceinline__ void table_stage(TableView<T>& a, int32_t na16, TableView<T>* b = nullptr, int32_t nb16 = 0) {
  extern __shared__ uint4 table_lds[];
  const uint4* __restrict__ sa = reinterpret_cast<const uint4*>(a.tab);
  for (int32_t k = threadIdx.x; k < na16; k += STAGE_THREADS) table_lds[k] = sa[k];
  a.tab = reinterpret_cast<const TableKnot<T>*>(table_lds);
  if (b) {
    const uint4* __restrict__ sb = reinterpret_cast<const uint4*>(b->tab);
    for (int32_t k = threadIdx.x; k < nb16; k += STAGE_THREADS) table_lds[na16 + k] = sb[k];
    b->tab = reinterpret_cast<const TableKnot<T>*>(table_lds + na16);
  }
  __syncthreads();
}

// n16: the table in 16-byte words (LDS instances).
template <typename T, bool HALF, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_table_forces(LjArgs<T, OFF> a, TableByPair<T> p, int32_t n16, T* __restrict__ f) {
  if constexpr (LDS) table_stage(p.v, n16);
  grid_rows(a.n, [&](int32_t row, int32_t lane) { lj_row_at<T, HALF, OFF, TRI>(a, p, f, row, lane); });
}
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_table_virial(LjArgs<T, OFF> a, TableByPair<T> p, int32_t n16, double ghost_w,
                                                                double* __restrict__ part) {
  if constexpr (LDS) table_stage(p.v, n16);
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}

using TableSet = nl_handle_s::TableSet;
size_t table_bytes(nl_handle_t h, const TableSet& ts) { return (size_t)ts.nslots * ts.nknots * 4 * (h->dtype == NL_F32 ? 4 : 8); }
// The tables of a launch go into LDS together where they fit and the set that decides was not made under NL_TABLE_LDS=0.
bool table_in_lds(const TableSet& ts, size_t bytes) { return ts.lds_env && bytes <= NL_TABLE_LDS_BYTES; }
// The view of a set in T: its scalars rounded to T once, as lj_scalars rounds its own.
template <typename T> TableView<T> table_view(const TableSet& ts, const void* tab, const int32_t* types) {
  return {static_cast<const TableKnot<T>*>(tab), (T)ts.x0, (T)ts.xc, (T)ts.iD, ts.nknots, ts.ntypes, ts.ntypes > 1 ? types : nullptr};
}
// the most blocks of the persistent grids over n rows
int32_t table_blocks(int32_t n) { return (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, NL_TABLE_BLOCKS); }

int table_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, void* f_dev, hipStream_t s, const uint32_t* status) {
  const size_t bytes = table_bytes(h, h->tb);
  return rows_launch(h, q_dev, stride, f_dev, 4, s, status, [&](auto i, const auto& a, auto* f) {
    using I = decltype(i);
    using T = typename I::T;
    const TableByPair<T> p = {table_view<T>(h->tb, h->tb.tab, h->ty_types)};
    with_flag(table_in_lds(h->tb, bytes), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_table_forces<T, I::half, typename I::OFF, I::tri, L>), dim3(table_blocks(a.n)), dim3(STAGE_THREADS), L ? bytes : 0, s, a, p,
                         (int32_t)(bytes / 16), f);
    });
  });
}

int table_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, double* out_dev, hipStream_t s, const uint32_t* status) {
  const size_t bytes = table_bytes(h, h->tb);
  const double ghost_w = h->plan.full ? 1.0 : 0.5;
  return totals_launch(h, q_dev, stride, out_dev, s, status, NL_TABLE_BLOCKS, [&](auto i, const auto& a, int32_t nblk, double* part) {
    using I = decltype(i);
    using T = typename I::T;
    const TableByPair<T> p = {table_view<T>(h->tb, h->tb.tab, h->ty_types)};
    with_flag(table_in_lds(h->tb, bytes), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_table_virial<T, typename I::OFF, I::tri, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bytes : 0, s, a, p, (int32_t)(bytes / 16),
                         ghost_w, part);
    });
    return NL_OK;
  });
}

// What the calls over a table need of the handle beyond consumer_ready: the set; with more than one type a type table of its
// ntypes; and a list that reaches its r_max (list_reach: a pair of types with rc_ab = 0 has no entries), less the skin for the
// enqueue variants.
int table_set_reach(nl_handle_t h, const TableSet& ts, double skin) {
  if (ts.nknots == 0) return fail(h, NL_ERR_STATE);
  if (ts.ntypes > 1) {
    if (!h->ty_types) return fail(h, NL_ERR_STATE);
    if (h->ty_ntypes != ts.ntypes) return fail(h, NL_ERR_ARG);
  }
  return ts.r_max <= list_reach(h, true) - skin ? NL_OK : fail(h, NL_ERR_ARG);
}
int table_reach(nl_handle_t h, double skin) { return table_set_reach(h, h->tb, skin); }

// The device form of one array pair in T: {V_k, dV_k, W_k, dW_k}, the differences taken in double and rounded once.
template <typename T> void table_knots(int64_t nslots, int32_t nknots, const double* V, const double* W, T* out) {
  for (int64_t sl = 0; sl < nslots; sl++)
    for (int32_t k = 0; k < nknots; k++) {
      const int64_t at = sl * nknots + k;
      const bool last = k == nknots - 1;
      out[4 * at + 0] = (T)V[at], out[4 * at + 1] = last ? (T)0 : (T)(V[at + 1] - V[at]);
      out[4 * at + 2] = (T)W[at], out[4 * at + 3] = last ? (T)0 : (T)(W[at + 1] - W[at]);
    }
}

// What a setter does once its scalar arguments are good: nseg array pairs {V, W} of [nslots][nknots] must be finite
// (NL_ERR_ARG); their knots go into ts.tab one behind the other in the position type; the first one's grid is the set's.
// Synchronous (the device may still replay a graph that reads the old tables; the enqueue variants copy nothing), and an
// error leaves the old set as it was.  NL_TABLE_LDS is read per set: one handle, and one list, can be walked on both paths.
struct TableSeg {
  int32_t nslots, nknots;
  const double *V, *W;
};
int table_upload(nl_handle_t h, TableSet& ts, int32_t ntypes, double r_min, double r_max, const TableSeg* seg, int nseg) {
  int64_t count = 0;
  for (int g = 0; g < nseg; g++) {
    const int64_t c = (int64_t)seg[g].nslots * seg[g].nknots;
    for (int64_t k = 0; k < c; k++)
      if (!std::isfinite(seg[g].V[k]) || !std::isfinite(seg[g].W[k])) return fail(h, NL_ERR_ARG);
    count += c;
  }
  HIPCHK(h, hipSetDevice(h->device));
  const bool f32 = h->dtype == NL_F32;
  const size_t bytes = (size_t)count * 4 * (f32 ? 4 : 8);
  std::vector<char> knots(bytes);
  for (int64_t g = 0, at = 0; g < nseg; at += (int64_t)seg[g].nslots * seg[g].nknots, g++) {
    if (f32) table_knots(seg[g].nslots, seg[g].nknots, seg[g].V, seg[g].W, reinterpret_cast<float*>(knots.data()) + 4 * at);
    else table_knots(seg[g].nslots, seg[g].nknots, seg[g].V, seg[g].W, reinterpret_cast<double*>(knots.data()) + 4 * at);
  }
  HIPCHK(h, hipDeviceSynchronize());
  if (!ts.tab.holds((int64_t)bytes))  // (no build touches it: side_alloc's kind, but the old table is kept on failure)
    if (int rc = hip_status(h, ts.tab.replace_keeping(bytes, (int64_t)bytes))) return rc;
  HIPCHK(h, hipMemcpy(ts.tab, knots.data(), bytes, hipMemcpyHostToDevice));
  const char* lds = getenv("NL_TABLE_LDS");
  ts.lds_env = !lds || atoi(lds) != 0;
  ts.ntypes = ntypes, ts.nslots = seg[0].nslots, ts.nknots = seg[0].nknots;
  ts.r_min = r_min, ts.r_max = r_max;
  ts.x0 = r_min * r_min, ts.xc = r_max * r_max, ts.iD = 1.0 / ((ts.xc - ts.x0) / (double)(ts.nknots - 1));
  return NL_OK;
}

}  // namespace

extern "C" {

int nl_set_pair_table(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min, double r_max, const double* F_host,
                      const double* U_host) {
  if (!h) return NL_ERR_ARG;
  if (nknots == 0 || (!F_host && !U_host)) {  // clear (the buffer stays: a captured graph may still read it)
    h->tb.nknots = 0, h->tb.ntypes = 0;
    return NL_OK;
  }
  if (!F_host || !U_host || nknots < 2 || nknots > NL_TABLE_MAX_KNOTS || ntypes < 1 || ntypes > NL_MAX_TYPES || !(r_min > 0) ||
      !(r_min < r_max) || !std::isfinite(r_max))
    return fail(h, NL_ERR_ARG);
  const TableSeg seg = {ntypes * (ntypes + 1) / 2, nknots, F_host, U_host};
  return table_upload(h, h->tb, ntypes, r_min, r_max, &seg, 1);
}

int nl_get_pair_table(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min, double* r_max) {
  if (!h) return NL_ERR_ARG;
  if (h->tb.nknots == 0) return fail(h, NL_ERR_STATE);
  if (ntypes) *ntypes = h->tb.ntypes;
  if (nknots) *nknots = h->tb.nknots;
  if (r_min) *r_min = h->tb.r_min;
  if (r_max) *r_max = h->tb.r_max;
  return NL_OK;
}

int nl_table_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, false, table_forces_launch, table_reach);
}
int nl_table_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, true, table_forces_launch, table_reach);
}
int nl_table_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, false, table_virial_launch, table_reach);
}
int nl_table_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, true, table_virial_launch, table_reach);
}

}  // extern "C"
