// nl_table.inc -- tabulated pair potentials (DESIGN.md section 8o): forces, per-particle energies and the totals of
// nl_virial.inc for any pair potential the caller has sampled (nl_set_pair_table), from the list of the last build.  The rule
// is stated at nl_set_pair_table in include/nl_hip.h.  A second pair function on the walk of section 8l: the rows, the image,
// the half list's reaction, the slab shares and the fixed summation order are lj_row_at's and lj_virial_rows' (TableByPair
// is their PAR), the launch arguments are lj_args' and the entry points' checks lj_call's, with the table's own reach.
// What is new is the grid of the forces: k_lj takes one block per 4 rows, which a block that first stages a table of 16 KiB
// cannot afford, so k_table_forces is persistent -- at most NL_TABLE_BLOCKS blocks, each stages the table once and its waves
// then walk the rows 4 blockIdx + wave, + 4 gridDim, ...  (k_table_virial: the grid lj_virial_rows has always had).
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

template <typename T> struct TableByPair {
  static constexpr bool lanes_meet = false, table = true;  // (every lane reads its own knot: nothing to exchange)
  const TableKnot<T>* tab;  // [nslots][nknots], in LDS or in global memory
  T x0, xc, iD;             // r_min^2, r_max^2, 1 / D
  int32_t nknots, ntypes;
  const int32_t* __restrict__ types;  // ntypes > 1: the handle's type table; else nullptr
  __device__ __forceinline__ int32_t row(int32_t row, int32_t) const {
    // (k_type_check: types < ntypes; the min keeps the slot inside the table whatever the type table holds)
    return types ? min(types[row] & (NL_MAX_TYPES - 1), ntypes - 1) : 0;
  }
  __device__ __forceinline__ const TableKnot<T>* entry(int32_t ti, int32_t j) const {
    if (!types) return tab;
    const int32_t tj = min(types[j] & (NL_MAX_TYPES - 1), ntypes - 1);
    const int32_t lo = min(ti, tj), hi = max(ti, tj);
    return tab + (size_t)(lo * (2 * ntypes - lo + 1) / 2 + (hi - lo)) * nknots;  // slot(a, b) of nl_pair_histogram_typed
  }
  // linear in r^2 between the knots: no square root, one knot read.  A pair within r_max but below r_min has no value: NaN.
  __device__ __forceinline__ void pair(const TableKnot<T>* slot, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    in = r2 < xc && r2 > (T)0;
    const T s = (r2 - x0) * iD;
    const bool below = r2 < x0;
    const int32_t k = in && !below ? min((int32_t)s, nknots - 2) : 0;  // (s >= 0 here; outside, knot 0 is read and dropped)
    const TableKnot<T> v = slot[k];
    const T t = s - (T)k;
    const T fr = in ? (below ? (T)NAN : v.F + t * v.dF) : (T)0;
    pe = in ? (below ? (T)NAN : v.U + t * v.dU) : (T)0;
    fx = fr * dx, fy = fr * dy, fz = fr * dz;
  }
};

// The table into the block's dynamic LDS, 16 bytes per thread and step; returns it.
template <typename T> __device__ __forceinline__ const TableKnot<T>* table_stage(const TableKnot<T>* __restrict__ g, int32_t n16) {
  extern __shared__ uint4 table_lds[];
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(g);
  for (int32_t k = threadIdx.x; k < n16; k += STAGE_THREADS) table_lds[k] = src[k];
  __syncthreads();
  return reinterpret_cast<const TableKnot<T>*>(table_lds);
}

// n16: the table in 16-byte words (LDS instances).
template <typename T, bool HALF, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_table_forces(LjArgs<T, OFF> a, TableByPair<T> p, int32_t n16, T* __restrict__ f) {
  if constexpr (LDS) p.tab = table_stage<T>(p.tab, n16);
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; row < a.n; row += (int32_t)gridDim.x * 4) lj_row_at<T, HALF, OFF, TRI>(a, p, f, row, lane);
}
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_table_virial(LjArgs<T, OFF> a, TableByPair<T> p, int32_t n16, double ghost_w,
                                                                double* __restrict__ part) {
  if constexpr (LDS) p.tab = table_stage<T>(p.tab, n16);
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}

size_t table_bytes(nl_handle_t h) {
  const size_t nslots = (size_t)h->tb_ntypes * (h->tb_ntypes + 1) / 2;
  return nslots * (size_t)h->tb_nknots * 4 * (h->dtype == NL_F32 ? 4 : 8);
}
bool table_in_lds(nl_handle_t h) { return h->tb_lds_env && table_bytes(h) <= NL_TABLE_LDS_BYTES; }
// The scalars rounded to T once, as lj_scalars rounds its own.
template <typename T> TableByPair<T> table_by_pair(nl_handle_t h) {
  return {static_cast<const TableKnot<T>*>(h->tb_tab), (T)h->tb_x0, (T)h->tb_xc, (T)h->tb_iD, h->tb_nknots, h->tb_ntypes,
          h->tb_ntypes > 1 ? h->ty_types.get() : nullptr};
}
// f(std::true_type or std::false_type) by v
template <typename F> void with_flag(bool v, F&& f) { v ? f(std::true_type()) : f(std::false_type()); }

int table_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, const double*, void* f_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, NL_TABLE_BLOCKS);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    const TableByPair<T> p = table_by_pair<T>(h);
    const size_t bytes = table_bytes(h);
    T* f = static_cast<T*>(f_dev);
    if (!h->plan.full) {
      const size_t count = 4 * (size_t)n;
      hipLaunchKernelGGL((k_lj_zero<T>), dim3((unsigned)std::min<size_t>((count + 255) / 256, 8192)), dim3(256), 0, s, f, count);
    }
    with_flag(!h->plan.full, [&](auto half) {
      with_flag(h->plan.tilt, [&](auto tri) {
        with_flag(table_in_lds(h), [&](auto lds) {
          constexpr bool H = decltype(half)::value, R = decltype(tri)::value, L = decltype(lds)::value;
          hipLaunchKernelGGL((k_table_forces<T, H, OFF, R, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bytes : 0, s, a, p, (int32_t)(bytes / 16), f);
        });
      });
    });
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

// virial_launch with the table's kernel in front of k_virial_reduce (vir_part and its first-call rule are shared).
int table_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, const double*, double* out_dev, hipStream_t s,
                        const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) {
    HIPCHK(h, hipMemsetAsync(out_dev, 0, sizeof(double) * VIR_OUT, s));
    return NL_OK;
  }
  if (int rc = virial_scratch(h, s)) return rc;
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, NL_TABLE_BLOCKS);
  double* part = h->vir_part;
  const double ghost_w = h->plan.full ? 1.0 : 0.5;
  const int rc = dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    const TableByPair<T> p = table_by_pair<T>(h);
    const size_t bytes = table_bytes(h);
    with_flag(h->plan.tilt, [&](auto tri) {
      with_flag(table_in_lds(h), [&](auto lds) {
        constexpr bool R = decltype(tri)::value, L = decltype(lds)::value;
        hipLaunchKernelGGL((k_table_virial<T, OFF, R, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bytes : 0, s, a, p, (int32_t)(bytes / 16), ghost_w, part);
      });
    });
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_virial_reduce, dim3(1), dim3(STAGE_THREADS), 0, s, part, nblk, h->plan.full ? 0.5 : 1.0, out_dev, status);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

// What the table calls need beyond consumer_ready: a table; with more than one slot a type table of its ntypes; and a list
// that reaches r_max -- rc, and with a type table every rc_ab > 0 (a pair of types with rc_ab = 0 has no entries) -- less the
// skin for the enqueue variants, whose list may be reused.
int table_reach(nl_handle_t h, double skin) {
  if (h->tb_nknots == 0) return fail(h, NL_ERR_STATE);
  if (h->tb_ntypes > 1) {
    if (!h->ty_types) return fail(h, NL_ERR_STATE);
    if (h->ty_ntypes != h->tb_ntypes) return fail(h, NL_ERR_ARG);
  }
  if (!(h->tb_rmax <= h->rc - skin)) return fail(h, NL_ERR_ARG);
  if (h->ty_types) {
    const int32_t nt = h->ty_ntypes;
    for (int32_t k = 0; k < nt * nt; k++)
      if (h->ty_rc[k] > 0.0 && !(h->tb_rmax <= h->ty_rc[k] - skin)) return fail(h, NL_ERR_ARG);
  }
  return NL_OK;
}

// The device form of one array pair in T: {F_k, dF_k, U_k, dU_k}, the differences taken in double and rounded once.
template <typename T> void table_knots(int64_t nslots, int32_t nknots, const double* F, const double* U, T* out) {
  for (int64_t sl = 0; sl < nslots; sl++)
    for (int32_t k = 0; k < nknots; k++) {
      const int64_t at = sl * nknots + k;
      const bool last = k == nknots - 1;
      out[4 * at + 0] = (T)F[at], out[4 * at + 1] = last ? (T)0 : (T)(F[at + 1] - F[at]);
      out[4 * at + 2] = (T)U[at], out[4 * at + 3] = last ? (T)0 : (T)(U[at + 1] - U[at]);
    }
}

}  // namespace

extern "C" {

int nl_set_pair_table(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min, double r_max, const double* F_host,
                      const double* U_host) {
  if (!h) return NL_ERR_ARG;
  if (nknots == 0 || (!F_host && !U_host)) {  // clear (the buffer stays: a captured graph may still read it)
    h->tb_nknots = 0, h->tb_ntypes = 0;
    return NL_OK;
  }
  if (!F_host || !U_host || nknots < 2 || nknots > NL_TABLE_MAX_KNOTS || ntypes < 1 || ntypes > NL_MAX_TYPES || !(r_min > 0) ||
      !(r_min < r_max) || !std::isfinite(r_max))
    return fail(h, NL_ERR_ARG);
  const int64_t nslots = (int64_t)ntypes * (ntypes + 1) / 2, count = nslots * nknots;
  for (int64_t k = 0; k < count; k++)
    if (!std::isfinite(F_host[k]) || !std::isfinite(U_host[k])) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  const bool f32 = h->dtype == NL_F32;
  const size_t bytes = (size_t)count * 4 * (f32 ? 4 : 8);
  std::vector<double> kd;
  std::vector<float> kf;
  if (f32) kf.resize(4 * (size_t)count), table_knots<float>(nslots, nknots, F_host, U_host, kf.data());
  else kd.resize(4 * (size_t)count), table_knots<double>(nslots, nknots, F_host, U_host, kd.data());
  // synchronous (the device may still replay a graph that reads the old table): the enqueue variants copy nothing
  HIPCHK(h, hipDeviceSynchronize());
  if (!h->tb_tab.holds((int64_t)bytes))  // (no build touches it: side_alloc's kind, but the old table is kept on failure)
    if (int rc = hip_status(h, h->tb_tab.replace_keeping(bytes, (int64_t)bytes))) return rc;
  HIPCHK(h, hipMemcpy(h->tb_tab, f32 ? (const void*)kf.data() : (const void*)kd.data(), bytes, hipMemcpyHostToDevice));
  const double x0 = r_min * r_min, xc = r_max * r_max;
  const char* lds = getenv("NL_TABLE_LDS");  // read per table: one handle, and one list, can be walked on both paths
  h->tb_lds_env = !lds || atoi(lds) != 0;
  h->tb_ntypes = ntypes, h->tb_nknots = nknots;
  h->tb_rmin = r_min, h->tb_rmax = r_max;
  h->tb_x0 = x0, h->tb_xc = xc, h->tb_iD = 1.0 / ((xc - x0) / (double)(nknots - 1));
  return NL_OK;
}

int nl_get_pair_table(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min, double* r_max) {
  if (!h) return NL_ERR_ARG;
  if (h->tb_nknots == 0) return fail(h, NL_ERR_STATE);
  if (ntypes) *ntypes = h->tb_ntypes;
  if (nknots) *nknots = h->tb_nknots;
  if (r_min) *r_min = h->tb_rmin;
  if (r_max) *r_max = h->tb_rmax;
  return NL_OK;
}

int nl_table_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return lj_call<void>(h, q_dev, q_stride, nullptr, f_dev, stream, false, table_forces_launch, table_reach);
}
int nl_table_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return lj_call<void>(h, q_dev, q_stride, nullptr, f_dev, stream, true, table_forces_launch, table_reach);
}
int nl_table_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return lj_call<double>(h, q_dev, q_stride, nullptr, out_dev, stream, false, table_virial_launch, table_reach);
}
int nl_table_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return lj_call<double>(h, q_dev, q_stride, nullptr, out_dev, stream, true, table_virial_launch, table_reach);
}

}  // extern "C"
