// nl_coul_excl.inc -- the excluded-pair term of the charges (DESIGN.md section 8v): E = sum over the pairs of the handle's
// exclusion table of q_i q_j C(r), the real-space correction an Ewald / PME sum owes for the bonded pairs that
// nl_set_exclusions took out of the list while the reciprocal sum still contains them (C = -prefactor erf(alpha r) / r:
// md_neighbor_list_amd/coulomb.py ewald_excluded).  The rule is stated at nl_set_coul_excl_table in include/nl_hip.h.
// The sum does not run over the list -- the pairs are not in it -- but over the exclusion CSR itself (ex_off, ex_ids of
// nl_exclude.inc), symmetric, so every row gathers its own force and nothing is scattered: no atomic anywhere.
// The walk is built for short rows.  An exclusion row holds 1 to a dozen ids; the consumers' wave per row (lj_row_pairs)
// would keep 2 to 8 of its 64 lanes busy.  Here a wave takes 8 consecutive rows, 8 lanes each (cx_row_pairs); lane g of a group
// walks the entries b + g, b + g + 8, ... of its row, the group's sums are closed by an xor tree over 4, 2, 1 and the group's
// first lane stores the row.  A block of STAGE_THREADS is 32 rows; both grids are persistent, so that a block stages the
// table into LDS once (table_stage of nl_table.inc) -- or reads it from global memory: the same knots, the same bits.
// What it shares: lj_image and consumer_call (nl_consumer.inc), TableView / TableSet / table_upload (nl_table.inc),
// vir_part, k_virial_reduce and the close of a block of lj_virial_rows (nl_virial.inc).
// Included at the end of nl_api.hip, behind nl_coulomb.inc.

namespace {

// The lanes of a row's group: 8.  tools/time_coul_excl.py builds a second library with -DNL_COUL_EXCL_LANES=64, the same sum on
// the consumers' wave per row (4 rows a block, the group's tree is wave_sum's), as the yardstick of its timings; the product
// is never built that way, and the rule of include/nl_hip.h is stated for 8.
#ifndef NL_COUL_EXCL_LANES
#define NL_COUL_EXCL_LANES 8
#endif
constexpr int CX_LANES = NL_COUL_EXCL_LANES;
constexpr int CX_ROWS = STAGE_THREADS / CX_LANES;         // rows of a block: 32
constexpr int CX_FORCE_BLOCKS = 8 * NL_COUL_EXCL_BLOCKS;  // most blocks of the forces (the totals: NL_COUL_EXCL_BLOCKS)
static_assert(NL_COUL_EXCL_BLOCKS <= VIR_BLOCKS, "k_coul_excl_virial leaves its partials in vir_part");
static_assert(WAVE % CX_LANES == 0 && (CX_LANES & (CX_LANES - 1)) == 0, "the xor tree of cx_group_sum closes groups inside a wave");

// What both kernels receive: the positions and charges of the caller, the exclusion table, the box and mask of the last
// build (lj_args' rule) and the table.
template <typename T> struct CoulExclArgs {
  const T* __restrict__ q;
  int32_t stride;
  const T* __restrict__ charge;
  const int32_t* __restrict__ ex_off;
  const int32_t* __restrict__ ex_ids;
  int32_t n;
  const uint32_t* __restrict__ status;
  T Lx, Ly, Lz, xy, xz, yz;
  TableView<T> c;
};

// The sum of a group of CX_LANES = 8 lanes, in every lane of it: lanes g and g ^ 4, then ^ 2, then ^ 1.
template <typename T> __device__ __forceinline__ T cx_group_sum(T v) {
#pragma unroll
  for (int d = CX_LANES / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

// Lane g's entries of one row: on_pair(dx, dy, dz, fc, ec) with the nearest image of d = r_i - r_j (lj_image: the pairs are
// in no list, so this is the image by itself) and the pair's values.  No cut-off: a pair outside [r_min, r_max) -- a
// coincident one and a NaN r2 included -- has no value, and fc and ec are NaN whatever the charges.
template <typename T, bool TRI, typename F>
__device__ __forceinline__ void cx_row_pairs(const CoulExclArgs<T>& a, int32_t row, int32_t g, F&& on_pair) {
  const int32_t b = a.ex_off[row], e = a.ex_off[row + 1];
  if (b + g >= e) return;  // (an empty row, or a lane past a short one: neither the position nor the charge is read)
  T xi, yi, zi;
  load_xyz(a.q, a.stride, row, xi, yi, zi);
  const T qi = a.charge[row];
  for (int32_t k = b + g; k < e; k += CX_LANES) {
    const int32_t j = a.ex_ids[k];
    T xj, yj, zj;
    load_xyz(a.q, a.stride, j, xj, yj, zj);
    const T qq = qi * a.charge[j];
    T dx, dy, dz;
    lj_image<T, TRI>(xi, yi, zi, xj, yj, zj, dx, dy, dz, a.Lx, a.Ly, a.Lz, a.xy, a.xz, a.yz);
    const T r2 = dx * dx + dy * dy + dz * dz;
    const bool in = r2 >= a.c.x0 && r2 < a.c.xc;
    const T s = (r2 - a.c.x0) * a.c.iD;
    const int32_t kn = in ? min((int32_t)s, a.c.nknots - 2) : 0;
    const TableKnot<T> v = a.c.tab[kn];
    const T t = s - (T)kn;
    const T fc = in ? qq * (v.F + t * v.dF) : (T)NAN;
    const T ec = in ? qq * (v.U + t * v.dU) : (T)NAN;
    on_pair(dx, dy, dz, fc, ec);
  }
}

// f = {fx, fy, fz, pe_i} of every row, pe_i half the row's ec; ADD: added to what f holds, one read-modify-write per row.
// A failed list (status, the enqueue variants) gives NaN rows, ADD or not.
template <typename T, bool TRI, bool LDS, bool ADD>
__global__ void __launch_bounds__(STAGE_THREADS) k_coul_excl_forces(CoulExclArgs<T> a, int32_t n16, T* __restrict__ f) {
  if constexpr (LDS) table_stage(a.c, n16);
  const int32_t g = threadIdx.x & (CX_LANES - 1);
  const bool dead = a.status && *a.status != 0u;  // (uniform over the launch)
  for (int32_t row = (int32_t)blockIdx.x * CX_ROWS + (int32_t)(threadIdx.x / CX_LANES); row < a.n; row += (int32_t)gridDim.x * CX_ROWS) {
    T ax = 0, ay = 0, az = 0, ae = 0;
    if (!dead)
      cx_row_pairs<T, TRI>(a, row, g, [&](T dx, T dy, T dz, T fc, T ec) { ax += fc * dx, ay += fc * dy, az += fc * dz, ae += (T)0.5 * ec; });
    ax = cx_group_sum(ax), ay = cx_group_sum(ay), az = cx_group_sum(az), ae = cx_group_sum(ae);
    if (g != 0) continue;
    T* o = f + (size_t)row * 4;
    if (dead) ax = ay = az = ae = (T)NAN;
    else if constexpr (ADD) ax += o[0], ay += o[1], az += o[2], ae += o[3];
    o[0] = ax, o[1] = ay, o[2] = az, o[3] = ae;
  }
}

// The 8 totals: every lane keeps its sums in double across all its rows (terms in T, converted: exact), every entry once --
// k_virial_reduce halves them, the table holds every pair in both rows.  The close of the block is lj_virial_rows'.
template <typename T, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_coul_excl_virial(CoulExclArgs<T> a, int32_t n16, double* __restrict__ part) {
  __shared__ double red[4][VIR_OUT];
  if constexpr (LDS) table_stage(a.c, n16);
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = threadIdx.x & (CX_LANES - 1);
  double acc[VIR_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool live = !(a.status && *a.status != 0u);  // (uniform over the launch; a failed list: k_virial_reduce writes the NaN)
  for (int32_t row = (int32_t)blockIdx.x * CX_ROWS + (int32_t)(threadIdx.x / CX_LANES); live && row < a.n; row += (int32_t)gridDim.x * CX_ROWS) {
    cx_row_pairs<T, TRI>(a, row, g, [&](T dx, T dy, T dz, T fc, T ec) {
      const T fx = fc * dx, fy = fc * dy, fz = fc * dz;
      const T wxx = fx * dx, wyy = fy * dy, wzz = fz * dz, wxy = fx * dy, wxz = fx * dz, wyz = fy * dz;
      acc[0] += (double)wxx, acc[1] += (double)wyy, acc[2] += (double)wzz;
      acc[3] += (double)wxy, acc[4] += (double)wxz, acc[5] += (double)wyz;
      acc[6] += (double)ec;
      acc[7] += (fc != fc || ec != ec) ? (double)NAN : 1.0;  // (a pair without a value: all 8 are NaN)
    });
  }
#pragma unroll
  for (int c = 0; c < VIR_OUT; c++) acc[c] = wave_sum(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < VIR_OUT; c++) red[wave][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < VIR_OUT) {
    const int c = threadIdx.x;
    part[(size_t)blockIdx.x * VIR_OUT + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  }
}

// ---- host side
bool cx_in_lds(nl_handle_t h) { return table_in_lds(h->cx, table_bytes(h, h->cx)); }
int32_t cx_blocks(int32_t n, int32_t most) { return (int32_t)std::min<int64_t>(((int64_t)n + CX_ROWS - 1) / CX_ROWS, most); }

template <typename T>
CoulExclArgs<T> cx_args(nl_handle_t h, const void* q_dev, int32_t stride, const void* charge_dev, const uint32_t* status) {
  const Box& b = h->plan.box;
  const int pbc = h->plan.pbc;
  return {static_cast<const T*>(q_dev), stride, static_cast<const T*>(charge_dev), h->ex_off, h->ex_ids, h->n_rows, status,
          (pbc & 1) ? (T)b.L[0] : (T)0, (pbc & 2) ? (T)b.L[1] : (T)0, (pbc & 4) ? (T)b.L[2] : (T)0, (T)b.xy, (T)b.xz, (T)b.yz,
          table_view<T>(h->cx, h->cx.tab, nullptr)};
}

// f(T(), tri, lds) with the position type of the handle, the tilt of the last build's box and the table's path
template <typename F> void cx_dispatch(nl_handle_t h, F&& f) {
  with_flag(h->plan.tilt, [&](auto tri) {
    with_flag(cx_in_lds(h), [&](auto lds) {
      if (h->dtype == NL_F32) f(float(), tri, lds);
      else f(double(), tri, lds);
    });
  });
}

int cx_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, const void* charge_dev, void* f_dev, bool add, hipStream_t s,
                     const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  const size_t bytes = table_bytes(h, h->cx);
  cx_dispatch(h, [&](auto t, auto tri, auto lds) {
    using T = decltype(t);
    constexpr bool TRI = decltype(tri)::value, L = decltype(lds)::value;
    const CoulExclArgs<T> a = cx_args<T>(h, q_dev, stride, charge_dev, status);
    with_flag(add, [&](auto ad) {
      hipLaunchKernelGGL((k_coul_excl_forces<T, TRI, L, decltype(ad)::value>), dim3(cx_blocks(n, CX_FORCE_BLOCKS)), dim3(STAGE_THREADS), L ? bytes : 0,
                         s, a, (int32_t)(bytes / 16), static_cast<T*>(f_dev));
    });
  });
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

int cx_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, const void* charge_dev, double* out_dev, hipStream_t s,
                     const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) {
    HIPCHK(h, hipMemsetAsync(out_dev, 0, sizeof(double) * VIR_OUT, s));
    return NL_OK;
  }
  if (int rc = first_call_scratch(h, h->vir_part, sizeof(double) * VIR_OUT * VIR_BLOCKS, s)) return rc;
  const int32_t nblk = cx_blocks(n, NL_COUL_EXCL_BLOCKS);
  const size_t bytes = table_bytes(h, h->cx);
  double* part = h->vir_part;
  cx_dispatch(h, [&](auto t, auto tri, auto lds) {
    using T = decltype(t);
    constexpr bool TRI = decltype(tri)::value, L = decltype(lds)::value;
    hipLaunchKernelGGL((k_coul_excl_virial<T, TRI, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bytes : 0, s,
                       cx_args<T>(h, q_dev, stride, charge_dev, status), (int32_t)(bytes / 16), part);
  });
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_virial_reduce, dim3(1), dim3(STAGE_THREADS), 0, s, part, nblk, 0.5, out_dev, status);  // (every pair in two rows)
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

// What the calls need beyond consumer_ready: a whole single-device build whose ids are its rows (a slab build's rows are not
// the table's, local ids or not; a distributed build's ids are the caller's), both tables, and an exclusion table of the
// build's n.  No reach: an excluded pair is owed its term wherever it is, and the skin asks for nothing.
int cx_ready(nl_handle_t h) {
  if (h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  if (!h->ex_ids || h->cx.nknots == 0) return fail(h, NL_ERR_STATE);
  if (h->n == 0) return NL_OK;                      // (no rows: nothing is read of the table)
  if (h->ex_n != h->n) return fail(h, NL_ERR_ARG);  // (a global table of more ids than the build has rows)
  return NL_OK;
}

template <typename LAUNCH>
int cx_call(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, const void* out_dev, void* stream, bool enqueue,
            LAUNCH&& launch) {
  return consumer_call(h, q_dev, q_stride, out_dev, charge_dev != nullptr, stream, enqueue, [&](double) { return cx_ready(h); }, launch);
}

}  // namespace

extern "C" {

int nl_set_coul_excl_table(nl_handle_t h, int32_t nknots, double r_min, double r_max, const double* K_host, const double* C_host) {
  if (!h) return NL_ERR_ARG;
  if (nknots == 0 || (!K_host && !C_host)) {  // clear (the buffer stays, as the charge table's)
    h->cx.nknots = 0, h->cx.ntypes = 0;
    return NL_OK;
  }
  if (!K_host || !C_host || nknots < 2 || nknots > NL_TABLE_MAX_KNOTS || !(r_min > 0) || !(r_min < r_max) || !std::isfinite(r_max))
    return fail(h, NL_ERR_ARG);
  const TableSeg seg = {1, nknots, K_host, C_host};
  return table_upload(h, h->cx, 1, r_min, r_max, &seg, 1);
}

int nl_get_coul_excl_table(nl_handle_t h, int32_t* nknots, double* r_min, double* r_max, int32_t* lds) {
  if (!h) return NL_ERR_ARG;
  if (h->cx.nknots == 0) return fail(h, NL_ERR_STATE);
  if (nknots) *nknots = h->cx.nknots;
  if (r_min) *r_min = h->cx.r_min;
  if (r_max) *r_max = h->cx.r_max;
  if (lds) *lds = cx_in_lds(h) ? 1 : 0;
  return NL_OK;
}

int nl_coul_excl_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, int add, void* stream) {
  return cx_call(h, q_dev, q_stride, charge_dev, f_dev, stream, false, [&](hipStream_t s, const uint32_t* status) {
    return cx_forces_launch(h, q_dev, q_stride, charge_dev, f_dev, add != 0, s, status);
  });
}
int nl_coul_excl_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, int add,
                                void* stream) {
  return cx_call(h, q_dev, q_stride, charge_dev, f_dev, stream, true, [&](hipStream_t s, const uint32_t* status) {
    return cx_forces_launch(h, q_dev, q_stride, charge_dev, f_dev, add != 0, s, status);
  });
}
int nl_coul_excl_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev, void* stream) {
  return cx_call(h, q_dev, q_stride, charge_dev, out_dev, stream, false, [&](hipStream_t s, const uint32_t* status) {
    return cx_virial_launch(h, q_dev, q_stride, charge_dev, out_dev, s, status);
  });
}
int nl_coul_excl_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev, void* stream) {
  return cx_call(h, q_dev, q_stride, charge_dev, out_dev, stream, true, [&](hipStream_t s, const uint32_t* status) {
    return cx_virial_launch(h, q_dev, q_stride, charge_dev, out_dev, s, status);
  });
}

}  // extern "C"
