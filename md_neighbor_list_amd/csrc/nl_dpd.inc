// nl_dpd.inc -- the DPD pair thermostat (DESIGN.md section 8x): F_ij = [ fr_phi(r) - gamma w(r)^2 (e . v_ij) + sigma w(r) xi_ij /
// sqrt(dt) ] e_ij over the list of the last build -- dissipative particle dynamics proper where phi is a soft conservative
// table, and the momentum-conserving, Galilean-invariant thermostat of any other pair potential.  The rule is stated at
// nl_set_dpd in include/nl_hip.h.  No pair table can carry it: the term needs v_i - v_j, and a random number per pair and
// step that both rows of a full list, a half list and both position types agree on.  So the weight is one table A = w(r) / r
// on a grid of its own (no square root per pair: w e = A d, w^2 (e . v) e = A^2 (d . v) d), the velocities are a second
// gathered array of three components, and the noise is a counter-based hash of (seed, step, min(i, j), max(i, j)) in 64-bit
// integers, the step read from a device word of the caller's: a captured MD step draws fresh noise at every replay.
// One more pair function on the walk of section 8l: DpdByPair is the PAR of lj_row_at and lj_virial_rows over the table
// pieces of nl_table.inc; the grid is grid_rows', the pair table is the handle's (nl_set_pair_table), the launches are
// rows_launch and totals_launch and the entry points go through consumer_call with dpd_reach.  What nl_set_dpd leaves on the
// device, in knots of T one behind the other: [nknots] {A, dA, 0, 0}, [nslots] {g, 0, sg, 0}, and one knot whose first 8 bytes
// are fin(seed).  The pair table, the weight table and the slot parameters are staged into LDS together where they fit
// NL_TABLE_LDS_BYTES, else all are read from global memory: the same knots, the same bits.
// Included at the end of nl_api.hip, behind nl_coul_excl.inc.

namespace {

// The finaliser of the pair noise (the mix of splitmix64), modulo 2^64.
__host__ __device__ __forceinline__ uint64_t dpd_fin(uint64_t z) {
  z ^= z >> 30, z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27, z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// row() keeps the row's types (of the pair table and of the slot parameters: either may have one type only), v_i and the row's
// half of the pair's key; entry() picks the phi slot, loads v_j and the slot's g and sg and draws xi; pair() is the rule.
template <typename T> struct DpdByPair {
  static constexpr bool lanes_meet = false, table = true;
  TableView<T> phi, w;       // the handle's pair table and the weight table (one slot; its ntypes and types: the parameters')
  const TableKnot<T>* par;   // [nslots] {g, -, sg, -}, behind the weight knots (dpd_begin)
  int32_t nslots;
  const T* __restrict__ v;   // n rows of v_stride T, the caller's
  int32_t v_stride;
  uint64_t key;              // fin(fin(seed) + step) of this launch (dpd_begin)
  struct Row {
    int32_t tp, td;
    uint32_t i;
    T vx, vy, vz;
  };
  struct Entry {
    const TableKnot<T>* phi;
    T dvx, dvy, dvz, g, sg, xi;
  };
  __device__ __forceinline__ Row row(int32_t row, int32_t) const {
    Row r = {type_of(phi.types, row, phi.ntypes), type_of(w.types, row, w.ntypes), (uint32_t)row, 0, 0, 0};
    load_xyz(v, v_stride, row, r.vx, r.vy, r.vz);
    return r;
  }
  __device__ __forceinline__ Entry entry(const Row& r, int32_t j) const {
    T vx, vy, vz;
    load_xyz(v, v_stride, j, vx, vy, vz);
    const TableKnot<T> sl = par[w.types ? pair_slot(r.td, type_of(w.types, j, w.ntypes), w.ntypes) : 0];
    // the same 24 bits from both rows of a pair: the key is symmetric in (i, j)
    const uint32_t lo = min(r.i, (uint32_t)j), hi = max(r.i, (uint32_t)j);
    const uint64_t z = dpd_fin(key + ((uint64_t)lo << 32 | (uint64_t)hi));
    const int32_t m = (int32_t)(z >> 40);
    const T xi = (T)(2 * m + 1 - (1 << 24)) * (T)(1.7320508075688772 / 16777216.0);  // (odd, |.| < 2^24: exact in fp32)
    return {phi.slot(r.tp, j), r.vx - vx, r.vy - vy, r.vz - vz, sl.F, sl.U, xi};
  }
  // Both reads spelled out, as CoulByPair::pair (section 8q).  A pair below the weight table is NaN whatever gamma and sigma:
  // the products are taken of the NaN, never skipped for g == 0, and its pe is NaN with it (the totals: all 8).
  __device__ __forceinline__ void pair(const Entry& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    const bool in_p = r2 < phi.xc && r2 > (T)0;
    const T sp = (r2 - phi.x0) * phi.iD;
    const bool below_p = r2 < phi.x0;
    const int32_t kp = in_p && !below_p ? min((int32_t)sp, phi.nknots - 2) : 0;
    const TableKnot<T> u = e.phi[kp];
    const T tp = sp - (T)kp;
    const T frp = in_p ? (below_p ? (T)NAN : u.F + tp * u.dF) : (T)0;
    const T pep = in_p ? (below_p ? (T)NAN : u.U + tp * u.dU) : (T)0;
    const bool in_d = r2 < w.xc && r2 > (T)0;
    const T sd = (r2 - w.x0) * w.iD;
    const bool below_d = r2 < w.x0;
    const int32_t kd = in_d && !below_d ? min((int32_t)sd, w.nknots - 2) : 0;
    const TableKnot<T> a = w.tab[kd];
    const T td = sd - (T)kd;
    const T A = below_d ? (T)NAN : a.F + td * a.dF;
    const T dot = (dx * e.dvx + dy * e.dvy) + dz * e.dvz;
    const T fd = -((e.g * (A * A)) * dot);
    const T fn = (e.sg * A) * e.xi;
    const T fdpd = in_d ? fd + fn : (T)0;
    const T fr = frp + fdpd;
    pe = in_d && below_d ? (T)NAN : pep;
    in = in_p || in_d;
    fx = fr * dx, fy = fr * dy, fz = fr * dz;
  }
};

// What a block does first: the launch's key, from two words every lane reads at the same address (one scalar load each, and
// the two 64-bit products in scalar registers: once per wave); the tables into LDS; the slot parameters behind the weight knots.
template <typename T, bool LDS>
__device__ __forceinline__ void dpd_begin(DpdByPair<T>& p, const uint64_t* __restrict__ step, int32_t n16_phi, int32_t n16_w) {
  const uint64_t seed_fin = *reinterpret_cast<const uint64_t*>(p.w.tab + p.w.nknots + p.nslots);
  p.key = dpd_fin(seed_fin + *step);
  if constexpr (LDS) table_stage(p.phi, n16_phi, &p.w, n16_w);
  p.par = p.w.tab + p.w.nknots;
}

template <typename T, bool HALF, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_dpd_forces(LjArgs<T, OFF> a, DpdByPair<T> p, const uint64_t* __restrict__ step, int32_t n16_phi,
                                                              int32_t n16_w, T* __restrict__ f) {
  dpd_begin<T, LDS>(p, step, n16_phi, n16_w);
  grid_rows(a.n, [&](int32_t row, int32_t lane) { lj_row_at<T, HALF, OFF, TRI>(a, p, f, row, lane); });
}
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_dpd_virial(LjArgs<T, OFF> a, DpdByPair<T> p, const uint64_t* __restrict__ step, int32_t n16_phi,
                                                              int32_t n16_w, double ghost_w, double* __restrict__ part) {
  dpd_begin<T, LDS>(p, step, n16_phi, n16_w);
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}

// ---- host side
// What a launch reads of the caller's beside the positions.
struct DpdIn {
  const void* v;
  int32_t v_stride;
  const uint64_t* step;
};

// the weight knots and the slot parameters: what is staged (the knot of the seed behind them is read once, from global memory)
size_t dpd_bytes(nl_handle_t h) { return ((size_t)h->dp.nknots + (size_t)h->dp_nslots) * 4 * (h->dtype == NL_F32 ? 4 : 8); }
// all three are staged, the pair table first; the DPD set decides (NL_TABLE_LDS at nl_set_dpd)
bool dpd_in_lds(nl_handle_t h) { return table_in_lds(h->dp, dpd_bytes(h) + table_bytes(h, h->tb)); }

template <typename T> DpdByPair<T> dpd_by_pair(nl_handle_t h, const DpdIn& in) {
  return {table_view<T>(h->tb, h->tb.tab, h->ty_types), table_view<T>(h->dp, h->dp.tab, h->ty_types), nullptr, h->dp_nslots,
          static_cast<const T*>(in.v), in.v_stride, 0};
}

int dpd_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, const DpdIn& in, void* f_dev, hipStream_t s, const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bw = dpd_bytes(h);
  return rows_launch(h, q_dev, stride, f_dev, 4, s, status, [&](auto i, const auto& a, auto* f) {
    using I = decltype(i);
    using T = typename I::T;
    with_flag(dpd_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_dpd_forces<T, I::half, typename I::OFF, I::tri, L>), dim3(table_blocks(a.n)), dim3(STAGE_THREADS), L ? bp + bw : 0, s, a,
                         dpd_by_pair<T>(h, in), in.step, (int32_t)(bp / 16), (int32_t)(bw / 16), f);
    });
  });
}

int dpd_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, const DpdIn& in, double* out_dev, hipStream_t s, const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bw = dpd_bytes(h);
  const double ghost_w = h->plan.full ? 1.0 : 0.5;
  return totals_launch(h, q_dev, stride, out_dev, s, status, NL_TABLE_BLOCKS, [&](auto i, const auto& a, int32_t nblk, double* part) {
    using I = decltype(i);
    using T = typename I::T;
    with_flag(dpd_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_dpd_virial<T, typename I::OFF, I::tri, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bp + bw : 0, s, a, dpd_by_pair<T>(h, in),
                         in.step, (int32_t)(bp / 16), (int32_t)(bw / 16), ghost_w, part);
    });
    return NL_OK;
  });
}

// Both sets, and a list that reaches the r_max of either (table_reach, table_set_reach: less the skin for the enqueue variants;
// the slot parameters' ntypes is the set's, so more than one type asks for a type table of exactly that ntypes).  The list must
// be a whole single-device build whose ids are its rows: the noise of a pair is keyed by its two rows, and the two ranks of a
// slab or distributed build would key a crossing pair by two different row pairs -- local-index slab lists are refused with the
// rest (eam_reach's condition).
int dpd_reach(nl_handle_t h, double skin) {
  if (h->dp.nknots == 0) return fail(h, NL_ERR_STATE);
  if (int rc = table_reach(h, skin)) return rc;
  if (h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  return table_set_reach(h, h->dp, skin);
}

// The four entry points: pair_call with the velocities and the step word as further arguments, neither of which may be NULL.
template <typename OUT>
int dpd_call(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride, const uint64_t* step_dev, OUT* out_dev,
             void* stream, bool enqueue, int (*launch)(nl_handle_t, const void*, int32_t, const DpdIn&, OUT*, hipStream_t, const uint32_t*)) {
  const DpdIn in = {v_dev, v_stride, step_dev};
  return consumer_call(h, q_dev, q_stride, out_dev, v_dev && step_dev && (v_stride == 3 || v_stride == 4), stream, enqueue,
                       [&](double skin) { return dpd_reach(h, skin); },
                       [&](hipStream_t s, const uint32_t* status) { return launch(h, q_dev, q_stride, in, out_dev, s, status); });
}

}  // namespace

extern "C" {

int nl_set_dpd(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min, double r_max, const double* A_host, const double* gamma_host,
               const double* sigma_host, double dt, uint64_t seed) {
  if (!h) return NL_ERR_ARG;
  if (nknots == 0 || (!A_host && !gamma_host && !sigma_host)) {  // clear (the buffer stays, as the pair table's)
    h->dp.nknots = 0, h->dp.ntypes = 0, h->dp_nslots = 0;
    return NL_OK;
  }
  if (!A_host || !gamma_host || !sigma_host || nknots < 2 || nknots > NL_TABLE_MAX_KNOTS || ntypes < 1 || ntypes > NL_MAX_TYPES || !(r_min > 0) ||
      !(r_min < r_max) || !std::isfinite(r_max) || !(dt > 0) || !std::isfinite(dt))
    return fail(h, NL_ERR_ARG);
  const int32_t nslots = ntypes * (ntypes + 1) / 2;
  std::vector<double> sg(nslots), zero(std::max(nknots, nslots), 0.0);
  const double rdt = std::sqrt(dt);
  for (int32_t k = 0; k < nslots; k++) {
    if (!(gamma_host[k] >= 0) || !(sigma_host[k] >= 0)) return fail(h, NL_ERR_ARG);
    sg[k] = sigma_host[k] / rdt;  // (in double; rounded to T once by the upload, which refuses what is not finite)
  }
  // the weight knots {A, dA, 0, 0}, the slots as single knots {g, 0, sg, 0}, and the knot that takes fin(seed)
  const TableSeg seg[3] = {{1, nknots, A_host, zero.data()}, {nslots, 1, gamma_host, sg.data()}, {1, 1, zero.data(), zero.data()}};
  if (int rc = table_upload(h, h->dp, ntypes, r_min, r_max, seg, 3)) return rc;
  h->dp_nslots = nslots, h->dp_dt = dt, h->dp_seed = seed;
  const uint64_t seed_fin = dpd_fin(seed);
  HIPCHK(h, hipMemcpy(static_cast<char*>(h->dp.tab.get()) + dpd_bytes(h), &seed_fin, sizeof seed_fin, hipMemcpyHostToDevice));
  return NL_OK;
}

int nl_get_dpd(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min, double* r_max, double* dt, uint64_t* seed, int32_t* lds) {
  if (!h) return NL_ERR_ARG;
  if (h->dp.nknots == 0) return fail(h, NL_ERR_STATE);
  if (ntypes) *ntypes = h->dp.ntypes;
  if (nknots) *nknots = h->dp.nknots;
  if (r_min) *r_min = h->dp.r_min;
  if (r_max) *r_max = h->dp.r_max;
  if (dt) *dt = h->dp_dt;
  if (seed) *seed = h->dp_seed;
  if (lds) *lds = h->tb.nknots != 0 && dpd_in_lds(h) ? 1 : 0;
  return NL_OK;
}

int nl_dpd_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride, const uint64_t* step_dev, void* f_dev,
                  void* stream) {
  return dpd_call(h, q_dev, q_stride, v_dev, v_stride, step_dev, f_dev, stream, false, dpd_forces_launch);
}
int nl_dpd_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride, const uint64_t* step_dev,
                          void* f_dev, void* stream) {
  return dpd_call(h, q_dev, q_stride, v_dev, v_stride, step_dev, f_dev, stream, true, dpd_forces_launch);
}
int nl_dpd_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride, const uint64_t* step_dev,
                  double* out_dev, void* stream) {
  return dpd_call(h, q_dev, q_stride, v_dev, v_stride, step_dev, out_dev, stream, false, dpd_virial_launch);
}
int nl_dpd_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride, const uint64_t* step_dev,
                          double* out_dev, void* stream) {
  return dpd_call(h, q_dev, q_stride, v_dev, v_stride, step_dev, out_dev, stream, true, dpd_virial_launch);
}

}  // extern "C"
