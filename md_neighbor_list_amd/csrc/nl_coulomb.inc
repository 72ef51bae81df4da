// nl_coulomb.inc -- per-particle charges (DESIGN.md section 8u): E = sum_pairs [ phi_{t_i t_j}(r) + q_i q_j C(r) ] over the list
// of the last build -- the real-space part of Ewald / PME, damped shifted force, Wolf, reaction field, Debye-Hueckel, whatever
// C(r) the caller has sampled (nl_set_coulomb_table; md_neighbor_list_amd/coulomb.py).  The rule is stated at
// nl_set_coulomb_table in include/nl_hip.h.  A pair table has a slot per pair of TYPES; a charge is a property of the
// particle, so the charge term cannot be a slot: it is one table C, K = -C'/r on a grid of its own, multiplied by the two
// charges of the entry, which the walk gathers beside the partner's position.
// One more pair function on the walk of section 8l: CoulByPair is the PAR of lj_row_at and lj_virial_rows over the table
// pieces of nl_table.inc (TableView, table_stage, TableSet, table_view, table_upload, table_set_reach); the grid is
// grid_rows', the pair table is the handle's (nl_set_pair_table), the launches are rows_launch and totals_launch and the
// entry points go through consumer_call with coul_reach.  The pair table and the charge table are staged into LDS together
// where they fit NL_TABLE_LDS_BYTES, else both are read from global memory: the same knots, the same bits.
// Included at the end of nl_api.hip, behind nl_sw.inc.

namespace {

// row() keeps the row's type (0 while the pair table has one slot) and q_i, entry() picks the phi slot and loads q_j,
// pair() is the rule.  The charge knots are TableKnot<T> with F := K = -C'(r) / r and U := C.
template <typename T> struct CoulByPair {
  static constexpr bool lanes_meet = false, table = true;
  TableView<T> phi, c;           // the handle's pair table and the charge table (one slot)
  const T* __restrict__ charge;  // one T per row of q, the caller's
  struct Row {
    int32_t tp;
    T q;
  };
  struct Entry {
    const TableKnot<T>* phi;
    T qq;
  };
  // (type_of on the view's fields, as EamByPair::row: section 8q)
  __device__ __forceinline__ Row row(int32_t row, int32_t) const { return {type_of(phi.types, row, phi.ntypes), charge[row]}; }
  __device__ __forceinline__ Entry entry(const Row& r, int32_t j) const { return {phi.slot(r.tp, j), r.q * charge[j]}; }
  // Both reads spelled out, as TableByPair::pair (section 8q).  A pair below the charge table is NaN whatever the charges:
  // the product with qq is taken of the NaN, never skipped for qq == 0.
  __device__ __forceinline__ void pair(const Entry& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    const bool in_p = r2 < phi.xc && r2 > (T)0;
    const T sp = (r2 - phi.x0) * phi.iD;
    const bool below_p = r2 < phi.x0;
    const int32_t kp = in_p && !below_p ? min((int32_t)sp, phi.nknots - 2) : 0;
    const TableKnot<T> w = e.phi[kp];
    const T tp = sp - (T)kp;
    const T frp = in_p ? (below_p ? (T)NAN : w.F + tp * w.dF) : (T)0;
    const T pep = in_p ? (below_p ? (T)NAN : w.U + tp * w.dU) : (T)0;
    const bool in_c = r2 < c.xc && r2 > (T)0;
    const T sc = (r2 - c.x0) * c.iD;
    const bool below_c = r2 < c.x0;
    const int32_t kc = in_c && !below_c ? min((int32_t)sc, c.nknots - 2) : 0;
    const TableKnot<T> v = c.tab[kc];
    const T tc = sc - (T)kc;
    const T fc = in_c ? e.qq * (below_c ? (T)NAN : v.F + tc * v.dF) : (T)0;
    const T ec = in_c ? e.qq * (below_c ? (T)NAN : v.U + tc * v.dU) : (T)0;
    const T fr = frp + fc;
    pe = pep + ec;
    in = in_p || in_c;
    fx = fr * dx, fy = fr * dy, fz = fr * dz;
  }
};

template <typename T, bool HALF, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_coul_forces(LjArgs<T, OFF> a, CoulByPair<T> p, int32_t n16_phi, int32_t n16_c, T* __restrict__ f) {
  if constexpr (LDS) table_stage(p.phi, n16_phi, &p.c, n16_c);
  grid_rows(a.n, [&](int32_t row, int32_t lane) { lj_row_at<T, HALF, OFF, TRI>(a, p, f, row, lane); });
}
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_coul_virial(LjArgs<T, OFF> a, CoulByPair<T> p, int32_t n16_phi, int32_t n16_c, double ghost_w,
                                                               double* __restrict__ part) {
  if constexpr (LDS) table_stage(p.phi, n16_phi, &p.c, n16_c);
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}

// ---- host side
// both tables are staged, the pair table first; the charge table's set decides (NL_TABLE_LDS at nl_set_coulomb_table)
bool coul_in_lds(nl_handle_t h) { return table_in_lds(h->cl, table_bytes(h, h->cl) + table_bytes(h, h->tb)); }

template <typename T> CoulByPair<T> coul_by_pair(nl_handle_t h, const void* charge_dev) {
  return {table_view<T>(h->tb, h->tb.tab, h->ty_types), table_view<T>(h->cl, h->cl.tab, nullptr), static_cast<const T*>(charge_dev)};
}

int coul_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, const void* charge_dev, void* f_dev, hipStream_t s,
                       const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bc = table_bytes(h, h->cl);
  return rows_launch(h, q_dev, stride, f_dev, 4, s, status, [&](auto i, const auto& a, auto* f) {
    using I = decltype(i);
    using T = typename I::T;
    with_flag(coul_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_coul_forces<T, I::half, typename I::OFF, I::tri, L>), dim3(table_blocks(a.n)), dim3(STAGE_THREADS), L ? bp + bc : 0, s, a,
                         coul_by_pair<T>(h, charge_dev), (int32_t)(bp / 16), (int32_t)(bc / 16), f);
    });
  });
}

int coul_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, const void* charge_dev, double* out_dev, hipStream_t s,
                       const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bc = table_bytes(h, h->cl);
  const double ghost_w = h->plan.full ? 1.0 : 0.5;
  return totals_launch(h, q_dev, stride, out_dev, s, status, NL_TABLE_BLOCKS, [&](auto i, const auto& a, int32_t nblk, double* part) {
    using I = decltype(i);
    using T = typename I::T;
    with_flag(coul_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_coul_virial<T, typename I::OFF, I::tri, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bp + bc : 0, s, a,
                         coul_by_pair<T>(h, charge_dev), (int32_t)(bp / 16), (int32_t)(bc / 16), ghost_w, part);
    });
    return NL_OK;
  });
}

// Both tables set, and a list that reaches the r_max of either (table_reach, table_set_reach: less the skin for the enqueue
// variants; a pair of types with rc_ab = 0 has no entries, and therefore no charge term either).  The list's ids must be rows
// of charge_dev as they are rows of q_dev: a list of caller ids (NL_GID_IN_W, a distributed build) is refused even where it
// is whole; consumer_ready has refused the slab builds made without nl_set_local_ids.
int coul_reach(nl_handle_t h, double skin) {
  if (h->cl.nknots == 0) return fail(h, NL_ERR_STATE);
  if (int rc = table_reach(h, skin)) return rc;
  if (h->args.gid || h->args.dyn) return fail(h, NL_ERR_STATE);
  return table_set_reach(h, h->cl, skin);
}

// The four entry points: pair_call with the charges as one more argument, which must not be NULL.
template <typename OUT>
int coul_call(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, OUT* out_dev, void* stream, bool enqueue,
              int (*launch)(nl_handle_t, const void*, int32_t, const void*, OUT*, hipStream_t, const uint32_t*)) {
  return consumer_call(h, q_dev, q_stride, out_dev, charge_dev != nullptr, stream, enqueue, [&](double skin) { return coul_reach(h, skin); },
                       [&](hipStream_t s, const uint32_t* status) { return launch(h, q_dev, q_stride, charge_dev, out_dev, s, status); });
}

}  // namespace

extern "C" {

int nl_set_coulomb_table(nl_handle_t h, int which, int32_t nknots, double r_min, double r_max, const double* K_host, const double* C_host) {
  if (!h) return NL_ERR_ARG;
  if (which != NL_COUL_LIST) return fail(h, NL_ERR_ARG);
  if (nknots == 0 || (!K_host && !C_host)) {  // clear (the buffer stays, as the pair table's)
    h->cl.nknots = 0, h->cl.ntypes = 0;
    return NL_OK;
  }
  if (!K_host || !C_host || nknots < 2 || nknots > NL_TABLE_MAX_KNOTS || !(r_min > 0) || !(r_min < r_max) || !std::isfinite(r_max))
    return fail(h, NL_ERR_ARG);
  const TableSeg seg = {1, nknots, K_host, C_host};
  return table_upload(h, h->cl, 1, r_min, r_max, &seg, 1);
}

int nl_get_coulomb_table(nl_handle_t h, int which, int32_t* nknots, double* r_min, double* r_max, int32_t* lds) {
  if (!h) return NL_ERR_ARG;
  if (which != NL_COUL_LIST) return fail(h, NL_ERR_ARG);
  if (h->cl.nknots == 0) return fail(h, NL_ERR_STATE);
  if (nknots) *nknots = h->cl.nknots;
  if (r_min) *r_min = h->cl.r_min;
  if (r_max) *r_max = h->cl.r_max;
  if (lds) *lds = h->tb.nknots != 0 && coul_in_lds(h) ? 1 : 0;
  return NL_OK;
}

int nl_coul_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, void* stream) {
  return coul_call(h, q_dev, q_stride, charge_dev, f_dev, stream, false, coul_forces_launch);
}
int nl_coul_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, void* stream) {
  return coul_call(h, q_dev, q_stride, charge_dev, f_dev, stream, true, coul_forces_launch);
}
int nl_coul_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev, void* stream) {
  return coul_call(h, q_dev, q_stride, charge_dev, out_dev, stream, false, coul_virial_launch);
}
int nl_coul_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev, void* stream) {
  return coul_call(h, q_dev, q_stride, charge_dev, out_dev, stream, true, coul_virial_launch);
}

}  // extern "C"
