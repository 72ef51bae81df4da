// nl_eam.inc -- embedded-atom potentials (DESIGN.md section 8p): E = sum_i F_{t_i}(rho_i) + sum_pairs phi(r) with
// rho_i = sum_j f_{t_j}(r_ij), from the list of the last build.  The rule is stated at nl_set_eam in include/nl_hip.h.  Three
// passes over the handle's per-particle scratch {rho, fp, Fe}:
//   k_eam_density   rho_i: lj_row_pairs with EamDensity as PAR (the image is the forces'); full list: a gather, half list:
//                   the partner's share by atomic after zero_async;
//   k_eam_embed     one thread per particle: Fe_i = F(rho_i) and fp_i = F'(rho_i) from the embedding table in global memory;
//   k_eam_forces / k_eam_virial   lj_row_at / lj_virial_rows with EamByPair as PAR: the pair table's fr, pe and the two
//                   density derivatives, fr = fr_phi + (fp_i G_j + fp_j G_i); then Fe_i goes into pe_i (k_eam_add_fe) or
//                   sum Fe_i into U (k_eam_fe_part, k_eam_add_u), each in one fixed order.
// Both pair functions are written over the table pieces of nl_table.inc (DESIGN.md section 8q): TableView with its knot, type
// and slot, table_stage, and on the host TableSet, table_view, table_upload and table_set_reach.  The grid is grid_rows',
// the pair table is the handle's (nl_set_pair_table), the launches are rows_launch and totals_launch and the entry points
// pair_call with eam_reach.  The pair table and the density table are staged into LDS together where they fit
// NL_TABLE_LDS_BYTES, else both are read from global memory: the same knots, the same bits.
// Included at the end of nl_api.hip, behind nl_table.inc.

namespace {

// sum Fe_i: one double per block of k_eam_fe_part, behind the partials of k_table_virial's grid in vir_part
static_assert((VIR_OUT + 1) * NL_TABLE_BLOCKS <= VIR_OUT * VIR_BLOCKS, "the partials of k_eam_fe_part behind those of k_eam_virial in vir_part");

// ---- pass 1: the densities.  The density knots are TableKnot<T> with F := G = -f'(r) / r and U := f, one slot per type of
// the SOURCE particle.  pair() gives the row's share f_{t_j} in pe and, for a half list, the partner's share f_{t_i} in fx.
template <typename T, bool HALF> struct EamDensity {
  static constexpr bool lanes_meet = false, table = true;
  TableView<T> v;
  struct Entry {
    const TableKnot<T>*sj, *si;
  };
  __device__ __forceinline__ int32_t row(int32_t row, int32_t) const { return v.type(row); }
  __device__ __forceinline__ Entry entry(int32_t ti, int32_t j) const {
    if (!v.types) return {v.tab, v.tab};
    return {v.slot(v.type(j)), v.slot(ti)};
  }
  __device__ __forceinline__ void pair(const Entry& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    const TableAt<T> g = v.knot(r2);
    in = g.in;
    const TableKnot<T> vj = e.sj[g.k];
    pe = in ? (g.below ? (T)NAN : vj.U + g.t * vj.dU) : (T)0;
    fx = fy = fz = (T)0;
    if constexpr (HALF) {
      const TableKnot<T> vi = e.si[g.k];
      fx = in ? (g.below ? (T)NAN : vi.U + g.t * vi.dU) : (T)0;
    }
  }
};

// one wave per row.  A list whose build failed (status) gives NaN densities, and with them NaN everywhere.
template <typename T, bool HALF, typename OFF, bool TRI>
__device__ __forceinline__ void eam_density_row(const LjArgs<T, OFF>& a, const EamDensity<T, HALF>& p, T* __restrict__ rho, int32_t row,
                                                int32_t lane) {
  if (a.status && *a.status != 0u) {  // (uniform: every row of the launch takes this branch, so no atomic follows the store)
    if (lane == 0) rho[row] = (T)NAN;
    return;
  }
  T acc = 0;
  lj_row_pairs<T, OFF, TRI>(a, p, row, lane, [&](int32_t j, LjPartner, T, T, T, T fi, T, T, T fj, bool in) {
    acc += fj;
    if (HALF && in) atomicAdd(&rho[j], fi);  // the stored pair once: the partner gathers the row's type
  });
  acc = wave_sum(acc);
  if (lane == 0) {
    if (HALF) atomicAdd(&rho[row], acc);
    else rho[row] = acc;
  }
}

template <typename T, bool HALF, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_eam_density(LjArgs<T, OFF> a, EamDensity<T, HALF> p, int32_t n16, T* __restrict__ rho) {
  if constexpr (LDS) table_stage(p.v, n16);
  grid_rows(a.n, [&](int32_t row, int32_t lane) { eam_density_row<T, HALF, OFF, TRI>(a, p, rho, row, lane); });
}

// ---- pass 2: the embedding.  Knots {E, dE, P, dP} (TableKnot<T> with F := E, U := P), uniform in rho on [0, rho_max], read
// from global memory: once per particle.  The domain rule is its own: rho outside [0, rho_max], or NaN, has no value.
template <typename T>
__global__ void __launch_bounds__(256) k_eam_embed(const T* __restrict__ rho, const TableKnot<T>* __restrict__ tab, const int32_t* __restrict__ types,
                                                   int32_t ntypes, int32_t nknots, T iDr, T rmax, int32_t n, T* __restrict__ fp, T* __restrict__ fe) {
  const int32_t i = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const T r = rho[i];
  const bool ok = r >= (T)0 && r <= rmax;
  const T s = r * iDr;
  const int32_t k = ok ? min((int32_t)s, nknots - 2) : 0;
  const T t = s - (T)k;
  const int32_t ty = type_of(types, i, ntypes);
  const TableKnot<T> v = tab[(size_t)ty * nknots + k];
  fe[i] = ok ? v.F + t * v.dF : (T)NAN;
  fp[i] = ok ? v.U + t * v.dU : (T)NAN;
}

// ---- pass 3: the pair function of the forces and the totals.  row() keeps the row's types and fp_i, entry() loads fp_j and
// picks the three slots, pair() is the rule.  The embedding term is taken only where the pair is within r_max_d (not as a
// product with 0), so a NaN fp reaches the partners within the density's range and nobody else.
template <typename T> struct EamByPair {
  static constexpr bool lanes_meet = false, table = true;
  TableView<T> phi, d;       // the handle's pair table and the density table
  const T* __restrict__ fp;  // F'(rho) of every particle (k_eam_embed)
  struct Row {
    int32_t tp, td;  // the row's type for the pair table (0 while that has one slot) and for the density table
    T fp;
  };
  struct Entry {
    const TableKnot<T>*phi, *di, *dj;
    T fpi, fpj;
  };
  // (type_of and the slots on the views' fields, not through TableView::type and slot(t): behind those the 32 instances of
  // k_eam_forces lose their parents' v_mad_i64_i32 for a 64-bit multiply, section 8q)
  __device__ __forceinline__ Row row(int32_t row, int32_t) const {
    return {type_of(phi.types, row, phi.ntypes), type_of(d.types, row, d.ntypes), fp[row]};
  }
  __device__ __forceinline__ Entry entry(const Row& r, int32_t j) const {
    const int32_t tj = type_of(d.types, j, d.ntypes);
    return {phi.slot(r.tp, j), d.tab + (size_t)r.td * d.nknots, d.tab + (size_t)tj * d.nknots, r.fp, fp[j]};
  }
  __device__ __forceinline__ void pair(const Entry& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    const TableAt<T> a = phi.knot(r2);
    const TableKnot<T> v = e.phi[a.k];
    const T frp = a.in ? (a.below ? (T)NAN : v.F + a.t * v.dF) : (T)0;
    pe = a.in ? (a.below ? (T)NAN : v.U + a.t * v.dU) : (T)0;
    const TableAt<T> g = d.knot(r2);
    const TableKnot<T> vi = e.di[g.k], vj = e.dj[g.k];
    const T Gi = g.below ? (T)NAN : vi.F + g.t * vi.dF, Gj = g.below ? (T)NAN : vj.F + g.t * vj.dF;
    const T emb = g.in ? e.fpi * Gj + e.fpj * Gi : (T)0;
    const T fr = frp + emb;
    in = a.in || g.in;
    fx = fr * dx, fy = fr * dy, fz = fr * dz;
  }
};

template <typename T, bool HALF, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_eam_forces(LjArgs<T, OFF> a, EamByPair<T> p, int32_t n16_phi, int32_t n16_d, T* __restrict__ f) {
  if constexpr (LDS) table_stage(p.phi, n16_phi, &p.d, n16_d);
  grid_rows(a.n, [&](int32_t row, int32_t lane) { lj_row_at<T, HALF, OFF, TRI>(a, p, f, row, lane); });
}
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_eam_virial(LjArgs<T, OFF> a, EamByPair<T> p, int32_t n16_phi, int32_t n16_d, double ghost_w,
                                                              double* __restrict__ part) {
  if constexpr (LDS) table_stage(p.phi, n16_phi, &p.d, n16_d);
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}

// pe_i += Fe_i: last, with one rounding, behind the half list's atomics as behind the full list's stores.
template <typename T> __global__ void __launch_bounds__(256) k_eam_add_fe(T* __restrict__ f, const T* __restrict__ fe, int32_t n) {
  const int32_t i = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) f[(size_t)i * 4 + 3] = f[(size_t)i * 4 + 3] + fe[i];
}

// sum Fe_i in double, one fixed order: thread g of the grid adds Fe_g, Fe_{g + threads}, ..., block_tree leaves one partial
// per block, and k_eam_add_u adds the partials as k_virial_reduce adds its own (thread t: t, t + 256, ...; the same tree,
// written out: behind block_tree this kernel reads out[6] through the scalar cache, section 8q) and puts the sum on U -- behind k_virial_reduce's factor 1/2 of a full list, which is for pairs.  A NaN Fe makes all 8 totals NaN.
template <typename T> __global__ void __launch_bounds__(STAGE_THREADS) k_eam_fe_part(const T* __restrict__ fe, int32_t n, double* __restrict__ part) {
  double s[1] = {0};
  for (int64_t i = (int64_t)blockIdx.x * STAGE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * STAGE_THREADS) s[0] += (double)fe[i];
  const auto& sm = block_tree(s);
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0][0];
}
__global__ void __launch_bounds__(STAGE_THREADS) k_eam_add_u(const double* __restrict__ part, int32_t nblk, double* __restrict__ out) {
  __shared__ double sm[STAGE_THREADS];
  const int32_t t = threadIdx.x;
  double s = 0;
  for (int32_t b = t; b < nblk; b += STAGE_THREADS) s += part[b];
  sm[t] = s;
  __syncthreads();
  for (int32_t d = STAGE_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) sm[t] += sm[t + d];
    __syncthreads();
  }
  const double fe = sm[0];
  if (t < VIR_OUT) {
    if (fe != fe) out[t] = (double)NAN;
    else if (t == 6) out[t] = out[t] + fe;
  }
}

// ---- host side
size_t eam_density_bytes(nl_handle_t h) { return table_bytes(h, h->ea); }
// the density pass stages its table alone; the forces and the totals stage it behind the pair table
bool eam_density_in_lds(nl_handle_t h) { return table_in_lds(h->ea, eam_density_bytes(h)); }
bool eam_forces_in_lds(nl_handle_t h) { return table_in_lds(h->ea, eam_density_bytes(h) + table_bytes(h, h->tb)); }

template <typename T> T* eam_rho(nl_handle_t h) { return static_cast<T*>(h->ea_part.get()); }
template <typename T> T* eam_fp(nl_handle_t h) { return eam_rho<T>(h) + h->n_max; }
template <typename T> T* eam_fe(nl_handle_t h) { return eam_rho<T>(h) + 2 * (size_t)h->n_max; }

// {rho, fp, Fe}: 3 T per particle of n_max, allocated by the first call of any of the four entry points; nl_initialize drops
// it with the other buffers sized by n_max.
int eam_scratch(nl_handle_t h, hipStream_t s) {
  return first_call_scratch(h, h->ea_part, 3 * ((size_t)h->n_max + 16) * (h->dtype == NL_F32 ? 4 : 8), s);
}

template <typename T> EamByPair<T> eam_by_pair(nl_handle_t h) {
  return {table_view<T>(h->tb, h->tb.tab, h->ty_types), table_view<T>(h->ea, h->ea.tab, h->ty_types), eam_fp<T>(h)};
}

// Passes 1 and 2 of a call: rho, then fp and Fe, of the n rows at the positions q.
int eam_density_launch(nl_handle_t h, const void* q_dev, int32_t stride, hipStream_t s, const uint32_t* status) {
  const size_t bytes = eam_density_bytes(h);
  return rows_launch(h, q_dev, stride, h->ea_part.get(), 1, s, status, [&](auto i, const auto& a, auto* rho) {
    using I = decltype(i);
    using T = typename I::T;
    const TableView<T> v = table_view<T>(h->ea, h->ea.tab, h->ty_types);
    with_flag(eam_density_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_eam_density<T, I::half, typename I::OFF, I::tri, L>), dim3(table_blocks(a.n)), dim3(STAGE_THREADS), L ? bytes : 0, s, a,
                         EamDensity<T, I::half>{v}, (int32_t)(bytes / 16), rho);
    });
    const TableKnot<T>* embed = reinterpret_cast<const TableKnot<T>*>(static_cast<const char*>(h->ea.tab.get()) + bytes);
    hipLaunchKernelGGL((k_eam_embed<T>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, rho, embed, v.types, h->ea.ntypes, h->ea_nke,
                       (T)h->ea_iDrho, (T)h->ea_rhomax, a.n, eam_fp<T>(h), eam_fe<T>(h));
  });
}

int eam_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, void* f_dev, hipStream_t s, const uint32_t* status) {
  if (h->n_rows == 0) return NL_OK;
  if (int rc = eam_scratch(h, s)) return rc;
  if (int rc = eam_density_launch(h, q_dev, stride, s, status)) return rc;
  const size_t bp = table_bytes(h, h->tb), bd = eam_density_bytes(h);
  return rows_launch(h, q_dev, stride, f_dev, 4, s, status, [&](auto i, const auto& a, auto* f) {
    using I = decltype(i);
    using T = typename I::T;
    with_flag(eam_forces_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_eam_forces<T, I::half, typename I::OFF, I::tri, L>), dim3(table_blocks(a.n)), dim3(STAGE_THREADS), L ? bp + bd : 0, s, a,
                         eam_by_pair<T>(h), (int32_t)(bp / 16), (int32_t)(bd / 16), f);
    });
    hipLaunchKernelGGL((k_eam_add_fe<T>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, f, eam_fe<T>(h), a.n);
  });
}

int eam_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, double* out_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  const int32_t nblk_fe = (int32_t)std::min<int64_t>(((int64_t)n + STAGE_THREADS - 1) / STAGE_THREADS, NL_TABLE_BLOCKS);
  const size_t bp = table_bytes(h, h->tb), bd = eam_density_bytes(h);
  const int rc = totals_launch(h, q_dev, stride, out_dev, s, status, NL_TABLE_BLOCKS, [&](auto i, const auto& a, int32_t nblk, double* part) -> int {
    using I = decltype(i);
    using T = typename I::T;
    if (int rs = eam_scratch(h, s)) return rs;
    if (int rd = eam_density_launch(h, q_dev, stride, s, status)) return rd;
    with_flag(eam_forces_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_eam_virial<T, typename I::OFF, I::tri, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bp + bd : 0, s, a, eam_by_pair<T>(h),
                         (int32_t)(bp / 16), (int32_t)(bd / 16), 1.0, part);
    });
    hipLaunchKernelGGL((k_eam_fe_part<T>), dim3(nblk_fe), dim3(STAGE_THREADS), 0, s, eam_fe<T>(h), n, part + (size_t)VIR_OUT * NL_TABLE_BLOCKS);
    return NL_OK;
  });
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(k_eam_add_u, dim3(1), dim3(STAGE_THREADS), 0, s, h->vir_part.get() + (size_t)VIR_OUT * NL_TABLE_BLOCKS, nblk_fe, out_dev);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

// The pair table's conditions, then the EAM tables' own: a whole single-device list (the force on an owned particle needs fp
// of its ghost partners: a forward halo exchange that is the caller's, so slab lists are refused, local-index ones included)
// under what table_set_reach asks for the density table.
int eam_reach(nl_handle_t h, double skin) {
  if (h->ea.nknots == 0) return fail(h, NL_ERR_STATE);
  if (int rc = table_reach(h, skin)) return rc;
  if (h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  return table_set_reach(h, h->ea, skin);
}

}  // namespace

extern "C" {

int nl_set_eam(nl_handle_t h, int32_t ntypes, int32_t nknots_d, double r_min_d, double r_max_d, const double* f_host, const double* G_host,
               int32_t nknots_e, double rho_max, const double* E_host, const double* P_host) {
  if (!h) return NL_ERR_ARG;
  if (nknots_d == 0 || nknots_e == 0 || (!f_host && !G_host && !E_host && !P_host)) {  // clear (the buffer stays, as the pair table's)
    h->ea.nknots = 0, h->ea_nke = 0, h->ea.ntypes = 0;
    return NL_OK;
  }
  if (!f_host || !G_host || !E_host || !P_host || nknots_d < 2 || nknots_d > NL_TABLE_MAX_KNOTS || nknots_e < 2 ||
      nknots_e > NL_TABLE_MAX_KNOTS || ntypes < 1 || ntypes > NL_MAX_TYPES || !(r_min_d > 0) || !(r_min_d < r_max_d) ||
      !std::isfinite(r_max_d) || !(rho_max > 0) || !std::isfinite(rho_max))
    return fail(h, NL_ERR_ARG);
  const TableSeg seg[2] = {{ntypes, nknots_d, G_host, f_host}, {ntypes, nknots_e, E_host, P_host}};
  if (int rc = table_upload(h, h->ea, ntypes, r_min_d, r_max_d, seg, 2)) return rc;
  h->ea_nke = nknots_e, h->ea_rhomax = rho_max;
  h->ea_iDrho = 1.0 / (rho_max / (double)(nknots_e - 1));
  return NL_OK;
}

int nl_get_eam(nl_handle_t h, int32_t* ntypes, int32_t* nknots_d, double* r_min_d, double* r_max_d, int32_t* nknots_e, double* rho_max,
               int32_t* lds_density, int32_t* lds_forces) {
  if (!h) return NL_ERR_ARG;
  if (h->ea.nknots == 0) return fail(h, NL_ERR_STATE);
  if (ntypes) *ntypes = h->ea.ntypes;
  if (nknots_d) *nknots_d = h->ea.nknots;
  if (r_min_d) *r_min_d = h->ea.r_min;
  if (r_max_d) *r_max_d = h->ea.r_max;
  if (nknots_e) *nknots_e = h->ea_nke;
  if (rho_max) *rho_max = h->ea_rhomax;
  if (lds_density) *lds_density = eam_density_in_lds(h) ? 1 : 0;
  if (lds_forces) *lds_forces = h->tb.nknots != 0 && eam_forces_in_lds(h) ? 1 : 0;
  return NL_OK;
}

int nl_eam_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, false, eam_forces_launch, eam_reach);
}
int nl_eam_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, true, eam_forces_launch, eam_reach);
}
int nl_eam_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, false, eam_virial_launch, eam_reach);
}
int nl_eam_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, true, eam_virial_launch, eam_reach);
}

int nl_eam_get_density(nl_handle_t h, const void** rho_dev, const void** fp_dev, int32_t* n) {
  if (!h || !rho_dev || !fp_dev || !n) return fail(h, NL_ERR_ARG);
  if (!h->ea_part) return fail(h, NL_ERR_STATE);
  const size_t sz = h->dtype == NL_F32 ? 4 : 8;
  *rho_dev = h->ea_part.get();
  *fp_dev = static_cast<const char*>(h->ea_part.get()) + sz * (size_t)h->n_max;
  *n = h->n_rows;
  return NL_OK;
}

}  // extern "C"
