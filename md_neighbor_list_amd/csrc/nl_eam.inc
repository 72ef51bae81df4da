// nl_eam.inc -- embedded-atom potentials (DESIGN.md section 8p): E = sum_i F_{t_i}(rho_i) + sum_pairs phi(r) with
// rho_i = sum_j f_{t_j}(r_ij), from the list of the last build.  The rule is stated at nl_set_eam in include/nl_hip.h.  Three
// passes over the handle's per-particle scratch {rho, fp, Fe}:
//   k_eam_density   rho_i: lj_row_pairs with EamDensity as PAR (the image is the forces'); full list: a gather, half list:
//                   the partner's share by atomic after k_lj_zero;
//   k_eam_embed     one thread per particle: Fe_i = F(rho_i) and fp_i = F'(rho_i) from the embedding table in global memory;
//   k_eam_forces / k_eam_virial   lj_row_at / lj_virial_rows with EamByPair as PAR: the pair table's fr, pe and the two
//                   density derivatives, fr = fr_phi + (fp_i G_j + fp_j G_i); then Fe_i goes into pe_i (k_eam_add_fe) or
//                   sum Fe_i into U (k_eam_fe_part, k_eam_add_u), each in one fixed order.
// The grid is the persistent one of nl_table.inc, the pair table is the handle's (nl_set_pair_table), the launch arguments
// are lj_args' and the entry points' checks lj_call's with eam_reach.  The pair table and the density table are staged into
// LDS together where they fit NL_TABLE_LDS_BYTES, else both are read from global memory: the same knots, the same bits.
// Included at the end of nl_api.hip, behind nl_table.inc.

namespace {

// sum Fe_i: one double per block of k_eam_fe_part, behind the partials of k_table_virial's grid in vir_part
static_assert((VIR_OUT + 1) * NL_TABLE_BLOCKS <= VIR_OUT * VIR_BLOCKS, "the partials of k_eam_fe_part behind those of k_eam_virial in vir_part");

// The knot of r2 on a grid uniform in r^2, as TableByPair::pair finds it: in, below, k and t.
template <typename T> struct EamKnot {
  bool in, below;
  int32_t k;
  T t;
};
template <typename T> __device__ __forceinline__ EamKnot<T> eam_knot(T r2, T x0, T xc, T iD, int32_t nknots) {
  const bool in = r2 < xc && r2 > (T)0;
  const T s = (r2 - x0) * iD;
  const bool below = r2 < x0;
  const int32_t k = in && !below ? min((int32_t)s, nknots - 2) : 0;  // (outside, knot 0 is read and dropped)
  return {in, below, k, s - (T)k};
}

// ---- pass 1: the densities.  The density knots are TableKnot<T> with F := G = -f'(r) / r and U := f, one slot per type of
// the SOURCE particle.  pair() gives the row's share f_{t_j} in pe and, for a half list, the partner's share f_{t_i} in fx.
template <typename T, bool HALF> struct EamDensity {
  static constexpr bool lanes_meet = false, table = true;
  const TableKnot<T>* tab;  // [ntypes][nknots], in LDS or in global memory
  T x0, xc, iD;
  int32_t nknots, ntypes;
  const int32_t* __restrict__ types;  // ntypes > 1: the handle's type table; else nullptr
  struct Entry {
    const TableKnot<T>*sj, *si;
  };
  __device__ __forceinline__ int32_t row(int32_t row, int32_t) const {
    return types ? min(types[row] & (NL_MAX_TYPES - 1), ntypes - 1) : 0;
  }
  __device__ __forceinline__ Entry entry(int32_t ti, int32_t j) const {
    if (!types) return {tab, tab};
    const int32_t tj = min(types[j] & (NL_MAX_TYPES - 1), ntypes - 1);
    return {tab + (size_t)tj * nknots, tab + (size_t)ti * nknots};
  }
  __device__ __forceinline__ void pair(const Entry& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    const EamKnot<T> g = eam_knot(r2, x0, xc, iD, nknots);
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
  if constexpr (LDS) p.tab = table_stage<T>(p.tab, n16);
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; row < a.n; row += (int32_t)gridDim.x * 4) eam_density_row<T, HALF, OFF, TRI>(a, p, rho, row, lane);
}

// ---- pass 2: the embedding.  Knots {E, dE, P, dP} (TableKnot<T> with F := E, U := P), uniform in rho on [0, rho_max], read
// from global memory: once per particle.  rho outside [0, rho_max], or NaN, has no value.
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
  const int32_t ty = types ? min(types[i] & (NL_MAX_TYPES - 1), ntypes - 1) : 0;
  const TableKnot<T> v = tab[(size_t)ty * nknots + k];
  fe[i] = ok ? v.F + t * v.dF : (T)NAN;
  fp[i] = ok ? v.U + t * v.dU : (T)NAN;
}

// ---- pass 3: the pair function of the forces and the totals.  row() keeps the row's types and fp_i, entry() loads fp_j and
// picks the three slots, pair() is the rule.  The embedding term is taken only where the pair is within r_max_d (not as a
// product with 0), so a NaN fp reaches the partners within the density's range and nobody else.
template <typename T> struct EamByPair {
  static constexpr bool lanes_meet = false, table = true;
  TableByPair<T> phi;        // the handle's pair table
  const TableKnot<T>* dtab;  // [dntypes][dnknots] density knots, in LDS or in global memory
  T dx0, dxc, diD;
  int32_t dnknots, dntypes;
  const int32_t* __restrict__ types;  // dntypes > 1: the handle's type table; else nullptr
  const T* __restrict__ fp;           // F'(rho) of every particle (k_eam_embed)
  struct Row {
    int32_t tp, td;  // the row's type for the pair table (0 while that has one slot) and for the density table
    T fp;
  };
  struct Entry {
    const TableKnot<T>*phi, *di, *dj;
    T fpi, fpj;
  };
  __device__ __forceinline__ Row row(int32_t row, int32_t lane) const {
    return {phi.row(row, lane), types ? min(types[row] & (NL_MAX_TYPES - 1), dntypes - 1) : 0, fp[row]};
  }
  __device__ __forceinline__ Entry entry(const Row& r, int32_t j) const {
    const int32_t tj = types ? min(types[j] & (NL_MAX_TYPES - 1), dntypes - 1) : 0;
    return {phi.entry(r.tp, j), dtab + (size_t)r.td * dnknots, dtab + (size_t)tj * dnknots, r.fp, fp[j]};
  }
  __device__ __forceinline__ void pair(const Entry& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    const EamKnot<T> a = eam_knot(r2, phi.x0, phi.xc, phi.iD, phi.nknots);
    const TableKnot<T> v = e.phi[a.k];
    const T frp = a.in ? (a.below ? (T)NAN : v.F + a.t * v.dF) : (T)0;
    pe = a.in ? (a.below ? (T)NAN : v.U + a.t * v.dU) : (T)0;
    const EamKnot<T> d = eam_knot(r2, dx0, dxc, diD, dnknots);
    const TableKnot<T> vi = e.di[d.k], vj = e.dj[d.k];
    const T Gi = d.below ? (T)NAN : vi.F + d.t * vi.dF, Gj = d.below ? (T)NAN : vj.F + d.t * vj.dF;
    const T emb = d.in ? e.fpi * Gj + e.fpj * Gi : (T)0;
    const T fr = frp + emb;
    in = a.in || d.in;
    fx = fr * dx, fy = fr * dy, fz = fr * dz;
  }
};

// Both tables into the block's dynamic LDS, the pair table first (table_stage's loop over the two sources).
template <typename T> __device__ __forceinline__ void eam_stage(EamByPair<T>& p, int32_t n16_phi, int32_t n16_d) {
  extern __shared__ uint4 table_lds[];
  const uint4* __restrict__ sp = reinterpret_cast<const uint4*>(p.phi.tab);
  const uint4* __restrict__ sd = reinterpret_cast<const uint4*>(p.dtab);
  for (int32_t k = threadIdx.x; k < n16_phi; k += STAGE_THREADS) table_lds[k] = sp[k];
  for (int32_t k = threadIdx.x; k < n16_d; k += STAGE_THREADS) table_lds[n16_phi + k] = sd[k];
  __syncthreads();
  p.phi.tab = reinterpret_cast<const TableKnot<T>*>(table_lds);
  p.dtab = reinterpret_cast<const TableKnot<T>*>(table_lds + n16_phi);
}

template <typename T, bool HALF, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_eam_forces(LjArgs<T, OFF> a, EamByPair<T> p, int32_t n16_phi, int32_t n16_d, T* __restrict__ f) {
  if constexpr (LDS) eam_stage<T>(p, n16_phi, n16_d);
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; row < a.n; row += (int32_t)gridDim.x * 4) lj_row_at<T, HALF, OFF, TRI>(a, p, f, row, lane);
}
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_eam_virial(LjArgs<T, OFF> a, EamByPair<T> p, int32_t n16_phi, int32_t n16_d, double ghost_w,
                                                              double* __restrict__ part) {
  if constexpr (LDS) eam_stage<T>(p, n16_phi, n16_d);
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}

// pe_i += Fe_i: last, with one rounding, behind the half list's atomics as behind the full list's stores.
template <typename T> __global__ void __launch_bounds__(256) k_eam_add_fe(T* __restrict__ f, const T* __restrict__ fe, int32_t n) {
  const int32_t i = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) f[(size_t)i * 4 + 3] = f[(size_t)i * 4 + 3] + fe[i];
}

// sum Fe_i in double, one fixed order: thread g of the grid adds Fe_g, Fe_{g + threads}, ..., a tree over the block's threads
// leaves one partial per block, and k_eam_add_u adds the partials as k_virial_reduce adds its own (thread t: t, t + 256, ...;
// a tree) and puts the sum on U -- behind k_virial_reduce's factor 1/2 of a full list, which is for pairs.  A NaN Fe makes all
// 8 totals NaN.
template <typename T> __global__ void __launch_bounds__(STAGE_THREADS) k_eam_fe_part(const T* __restrict__ fe, int32_t n, double* __restrict__ part) {
  __shared__ double sm[STAGE_THREADS];
  const int32_t t = threadIdx.x;
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * STAGE_THREADS + t; i < n; i += (int64_t)gridDim.x * STAGE_THREADS) s += (double)fe[i];
  sm[t] = s;
  __syncthreads();
  for (int32_t d = STAGE_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) sm[t] += sm[t + d];
    __syncthreads();
  }
  if (t == 0) part[blockIdx.x] = sm[0];
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
size_t eam_knot_bytes(nl_handle_t h) { return 4 * (size_t)(h->dtype == NL_F32 ? 4 : 8); }
size_t eam_density_bytes(nl_handle_t h) { return (size_t)h->ea_ntypes * h->ea_nkd * eam_knot_bytes(h); }
// the density pass stages its table alone; the forces and the totals stage it behind the pair table
bool eam_density_in_lds(nl_handle_t h) { return h->ea_lds_env && eam_density_bytes(h) <= NL_TABLE_LDS_BYTES; }
bool eam_forces_in_lds(nl_handle_t h) { return h->ea_lds_env && eam_density_bytes(h) + table_bytes(h) <= NL_TABLE_LDS_BYTES; }
const char* eam_embed_tab(nl_handle_t h) { return static_cast<const char*>(h->ea_tab.get()) + eam_density_bytes(h); }

template <typename T> T* eam_rho(nl_handle_t h) { return static_cast<T*>(h->ea_part.get()); }
template <typename T> T* eam_fp(nl_handle_t h) { return eam_rho<T>(h) + h->n_max; }
template <typename T> T* eam_fe(nl_handle_t h) { return eam_rho<T>(h) + 2 * (size_t)h->n_max; }

// {rho, fp, Fe}: 3 T per particle of n_max, allocated by the first call of any of the four entry points (virial_scratch's
// rule: a stream that is being captured cannot allocate); nl_initialize drops it with the other buffers sized by n_max.
int eam_scratch(nl_handle_t h, hipStream_t s) {
  if (h->ea_part) return NL_OK;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIPCHK(h, hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) return fail(h, NL_ERR_STATE);
  return side_alloc(h, h->ea_part, 3 * ((size_t)h->n_max + 16) * (h->dtype == NL_F32 ? 4 : 8));
}

template <typename T> EamByPair<T> eam_by_pair(nl_handle_t h) {
  return {table_by_pair<T>(h), static_cast<const TableKnot<T>*>(h->ea_tab.get()), (T)h->ea_x0, (T)h->ea_xc, (T)h->ea_iD, h->ea_nkd, h->ea_ntypes,
          h->ea_ntypes > 1 ? h->ty_types.get() : nullptr, eam_fp<T>(h)};
}

// Passes 1 and 2 of a call: rho, then fp and Fe, of the n rows at the positions q.
template <typename T, typename OFF> int eam_density_launch(nl_handle_t h, const LjArgs<T, OFF>& a, hipStream_t s) {
  const int32_t n = h->n_rows;
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, NL_TABLE_BLOCKS);
  const int32_t* types = h->ea_ntypes > 1 ? h->ty_types.get() : nullptr;
  const TableKnot<T>* dtab = static_cast<const TableKnot<T>*>(h->ea_tab.get());
  const size_t bytes = eam_density_bytes(h);
  T* rho = eam_rho<T>(h);
  if (!h->plan.full)
    hipLaunchKernelGGL((k_lj_zero<T>), dim3((unsigned)std::min<size_t>(((size_t)n + 255) / 256, 8192)), dim3(256), 0, s, rho, (size_t)n);
  with_flag(!h->plan.full, [&](auto half) {
    with_flag(h->plan.tilt, [&](auto tri) {
      with_flag(eam_density_in_lds(h), [&](auto lds) {
        constexpr bool H = decltype(half)::value, R = decltype(tri)::value, L = decltype(lds)::value;
        const EamDensity<T, H> p = {dtab, (T)h->ea_x0, (T)h->ea_xc, (T)h->ea_iD, h->ea_nkd, h->ea_ntypes, types};
        hipLaunchKernelGGL((k_eam_density<T, H, OFF, R, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bytes : 0, s, a, p, (int32_t)(bytes / 16), rho);
      });
    });
  });
  hipLaunchKernelGGL((k_eam_embed<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rho, reinterpret_cast<const TableKnot<T>*>(eam_embed_tab(h)),
                     types, h->ea_ntypes, h->ea_nke, (T)h->ea_iDrho, (T)h->ea_rhomax, n, eam_fp<T>(h), eam_fe<T>(h));
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

int eam_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, const double*, void* f_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  if (int rc = eam_scratch(h, s)) return rc;
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, NL_TABLE_BLOCKS);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    if (int rc = eam_density_launch<T, OFF>(h, a, s)) return rc;
    const EamByPair<T> p = eam_by_pair<T>(h);
    const size_t bp = table_bytes(h), bd = eam_density_bytes(h);
    T* f = static_cast<T*>(f_dev);
    if (!h->plan.full) {
      const size_t count = 4 * (size_t)n;
      hipLaunchKernelGGL((k_lj_zero<T>), dim3((unsigned)std::min<size_t>((count + 255) / 256, 8192)), dim3(256), 0, s, f, count);
    }
    with_flag(!h->plan.full, [&](auto half) {
      with_flag(h->plan.tilt, [&](auto tri) {
        with_flag(eam_forces_in_lds(h), [&](auto lds) {
          constexpr bool H = decltype(half)::value, R = decltype(tri)::value, L = decltype(lds)::value;
          hipLaunchKernelGGL((k_eam_forces<T, H, OFF, R, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bp + bd : 0, s, a, p, (int32_t)(bp / 16),
                             (int32_t)(bd / 16), f);
        });
      });
    });
    hipLaunchKernelGGL((k_eam_add_fe<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, f, eam_fe<T>(h), n);
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

int eam_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, const double*, double* out_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) {
    HIPCHK(h, hipMemsetAsync(out_dev, 0, sizeof(double) * VIR_OUT, s));
    return NL_OK;
  }
  if (int rc = virial_scratch(h, s)) return rc;
  if (int rc = eam_scratch(h, s)) return rc;
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, NL_TABLE_BLOCKS);
  const int32_t nblk_fe = (int32_t)std::min<int64_t>(((int64_t)n + STAGE_THREADS - 1) / STAGE_THREADS, NL_TABLE_BLOCKS);
  double* part = h->vir_part;
  double* part_fe = part + (size_t)VIR_OUT * NL_TABLE_BLOCKS;
  const int rc = dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    if (int rc = eam_density_launch<T, OFF>(h, a, s)) return rc;
    const EamByPair<T> p = eam_by_pair<T>(h);
    const size_t bp = table_bytes(h), bd = eam_density_bytes(h);
    with_flag(h->plan.tilt, [&](auto tri) {
      with_flag(eam_forces_in_lds(h), [&](auto lds) {
        constexpr bool R = decltype(tri)::value, L = decltype(lds)::value;
        hipLaunchKernelGGL((k_eam_virial<T, OFF, R, L>), dim3(nblk), dim3(STAGE_THREADS), L ? bp + bd : 0, s, a, p, (int32_t)(bp / 16),
                           (int32_t)(bd / 16), 1.0, part);
      });
    });
    hipLaunchKernelGGL((k_eam_fe_part<T>), dim3(nblk_fe), dim3(STAGE_THREADS), 0, s, eam_fe<T>(h), n, part_fe);
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_virial_reduce, dim3(1), dim3(STAGE_THREADS), 0, s, part, nblk, h->plan.full ? 0.5 : 1.0, out_dev, status);
  hipLaunchKernelGGL(k_eam_add_u, dim3(1), dim3(STAGE_THREADS), 0, s, part_fe, nblk_fe, out_dev);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

// table_reach, extended: the pair table's conditions, then the EAM tables' own -- set; with more than one type a type table
// of that ntypes; a whole single-device list (the force on an owned particle needs fp of its ghost partners: a forward halo
// exchange that is the caller's, so slab lists are refused, local-index ones included); and a list that reaches r_max_d.
int eam_reach(nl_handle_t h, double skin) {
  if (h->ea_nkd == 0) return fail(h, NL_ERR_STATE);
  if (int rc = table_reach(h, skin)) return rc;
  if (h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  if (h->ea_ntypes > 1) {
    if (!h->ty_types) return fail(h, NL_ERR_STATE);
    if (h->ty_ntypes != h->ea_ntypes) return fail(h, NL_ERR_ARG);
  }
  if (!(h->ea_rmax <= h->rc - skin)) return fail(h, NL_ERR_ARG);
  if (h->ty_types) {
    const int32_t nt = h->ty_ntypes;
    for (int32_t k = 0; k < nt * nt; k++)
      if (h->ty_rc[k] > 0.0 && !(h->ea_rmax <= h->ty_rc[k] - skin)) return fail(h, NL_ERR_ARG);
  }
  return NL_OK;
}

}  // namespace

extern "C" {

int nl_set_eam(nl_handle_t h, int32_t ntypes, int32_t nknots_d, double r_min_d, double r_max_d, const double* f_host, const double* G_host,
               int32_t nknots_e, double rho_max, const double* E_host, const double* P_host) {
  if (!h) return NL_ERR_ARG;
  if (nknots_d == 0 || nknots_e == 0 || (!f_host && !G_host && !E_host && !P_host)) {  // clear (the buffer stays, as the pair table's)
    h->ea_nkd = 0, h->ea_nke = 0, h->ea_ntypes = 0;
    return NL_OK;
  }
  if (!f_host || !G_host || !E_host || !P_host || nknots_d < 2 || nknots_d > NL_TABLE_MAX_KNOTS || nknots_e < 2 ||
      nknots_e > NL_TABLE_MAX_KNOTS || ntypes < 1 || ntypes > NL_MAX_TYPES || !(r_min_d > 0) || !(r_min_d < r_max_d) ||
      !std::isfinite(r_max_d) || !(rho_max > 0) || !std::isfinite(rho_max))
    return fail(h, NL_ERR_ARG);
  const int64_t cd = (int64_t)ntypes * nknots_d, ce = (int64_t)ntypes * nknots_e;
  for (int64_t k = 0; k < cd; k++)
    if (!std::isfinite(f_host[k]) || !std::isfinite(G_host[k])) return fail(h, NL_ERR_ARG);
  for (int64_t k = 0; k < ce; k++)
    if (!std::isfinite(E_host[k]) || !std::isfinite(P_host[k])) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  const bool f32 = h->dtype == NL_F32;
  const size_t bytes = (size_t)(cd + ce) * 4 * (f32 ? 4 : 8);
  std::vector<double> kd;
  std::vector<float> kf;
  if (f32) {
    kf.resize(4 * (size_t)(cd + ce));
    table_knots<float>(ntypes, nknots_d, G_host, f_host, kf.data());
    table_knots<float>(ntypes, nknots_e, E_host, P_host, kf.data() + 4 * cd);
  } else {
    kd.resize(4 * (size_t)(cd + ce));
    table_knots<double>(ntypes, nknots_d, G_host, f_host, kd.data());
    table_knots<double>(ntypes, nknots_e, E_host, P_host, kd.data() + 4 * cd);
  }
  HIPCHK(h, hipDeviceSynchronize());  // synchronous, as nl_set_pair_table: a graph may still read the old tables
  if (!h->ea_tab.holds((int64_t)bytes))
    if (int rc = hip_status(h, h->ea_tab.replace_keeping(bytes, (int64_t)bytes))) return rc;
  HIPCHK(h, hipMemcpy(h->ea_tab, f32 ? (const void*)kf.data() : (const void*)kd.data(), bytes, hipMemcpyHostToDevice));
  const double x0 = r_min_d * r_min_d, xc = r_max_d * r_max_d;
  const char* lds = getenv("NL_TABLE_LDS");  // read per set, as for the pair table
  h->ea_lds_env = !lds || atoi(lds) != 0;
  h->ea_ntypes = ntypes, h->ea_nkd = nknots_d, h->ea_nke = nknots_e;
  h->ea_rmin = r_min_d, h->ea_rmax = r_max_d, h->ea_rhomax = rho_max;
  h->ea_x0 = x0, h->ea_xc = xc, h->ea_iD = 1.0 / ((xc - x0) / (double)(nknots_d - 1));
  h->ea_iDrho = 1.0 / (rho_max / (double)(nknots_e - 1));
  return NL_OK;
}

int nl_get_eam(nl_handle_t h, int32_t* ntypes, int32_t* nknots_d, double* r_min_d, double* r_max_d, int32_t* nknots_e, double* rho_max,
               int32_t* lds_density, int32_t* lds_forces) {
  if (!h) return NL_ERR_ARG;
  if (h->ea_nkd == 0) return fail(h, NL_ERR_STATE);
  if (ntypes) *ntypes = h->ea_ntypes;
  if (nknots_d) *nknots_d = h->ea_nkd;
  if (r_min_d) *r_min_d = h->ea_rmin;
  if (r_max_d) *r_max_d = h->ea_rmax;
  if (nknots_e) *nknots_e = h->ea_nke;
  if (rho_max) *rho_max = h->ea_rhomax;
  if (lds_density) *lds_density = eam_density_in_lds(h) ? 1 : 0;
  if (lds_forces) *lds_forces = h->tb_nknots != 0 && eam_forces_in_lds(h) ? 1 : 0;
  return NL_OK;
}

int nl_eam_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return lj_call<void>(h, q_dev, q_stride, nullptr, f_dev, stream, false, eam_forces_launch, eam_reach);
}
int nl_eam_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return lj_call<void>(h, q_dev, q_stride, nullptr, f_dev, stream, true, eam_forces_launch, eam_reach);
}
int nl_eam_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return lj_call<double>(h, q_dev, q_stride, nullptr, out_dev, stream, false, eam_virial_launch, eam_reach);
}
int nl_eam_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return lj_call<double>(h, q_dev, q_stride, nullptr, out_dev, stream, true, eam_virial_launch, eam_reach);
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
