// nl_sw.inc -- Stillinger-Weber three-body potentials (DESIGN.md section 8r): E = sum_pairs phi(r) + sum_i sum_{j<k}
// Lambda (cos theta_jik - c0)^2 g(r_ij) g(r_ik), from the full list of the last build.  The rule is stated at nl_set_sw in
// include/nl_hip.h.  The first consumer whose hot loop is not one pass over a row: one wave per centre row
//   1. walks the row with lj_row_pairs and SwPair (the pair table's arithmetic; in = in_phi || in_3): the row's pair force and
//      half energy as lj_row_at sums them (the totals: as lj_virial_rows), and in the same visit the in_3 partners {j, a} are
//      compacted into the wave's LDS strip at m + lanes_below(ballot) -- a write under EXEC, so the walk's divergent last chunk
//      needs no lane to stay;
//   2. lanes 0 .. m - 1 take a partner each from the strip and compute ir, g, G and their 4 x {Lambda, c0} of (t_i, t_j, *);
//   3. loops k = 0 .. m - 1, lane k's {b, ir_b, g_b, t_k} broadcast with v_readlane (k is uniform): lane j keeps only its own end,
//      sa += ca, sb += cb b, e += h for k != j, so no two lanes add to one accumulator;
//   4. F_j = sb - sa a; forces: F_j and e_j / 3 to f[j] by atomics, the row's own values (pair part + F_i, F_i = -wave_sum(F_j);
//      half pair energy + wave_sum(e) / 6) by lane 0's atomics on the zeroed f; totals: -a_c F_j,d doubled (exact) and e_j into
//      the lane's double sums, no atomic, block partials for k_virial_reduce (whose 1/2 of a full list then leaves every triple
//      once).
// m > NL_SW_MAX_NEAR: NaN to the centre, its in_3 partners (one more walk) and all 8 totals.
// The pieces are those of nl_table.inc and nl_consumer.inc (DESIGN.md section 8q): TableView, table_stage, TableSet, table_upload,
// table_set_reach, grid_rows, table_blocks, rows_launch, totals_launch, pair_call.  The pair table and the g tables are staged
// into LDS together where they fit NL_TABLE_LDS_BYTES with the block's strips, else both are read from global memory; the strips
// lie behind the tables in the block's dynamic LDS either way.
// Included at the end of nl_api.hip, behind nl_eam.inc.

namespace {

static_assert(NL_SW_MAX_NEAR == WAVE, "one in-range partner per lane");
static_assert(NL_SW_MAX_TYPES == 4, "a lane keeps {Lambda, c0} of its (t_i, t_j, 0 .. 3) in registers");

// The pair function of the walk: TableByPair's text on the pair table, and in = in_phi || in_3 for the pair count.
template <typename T> struct SwPair {
  static constexpr bool lanes_meet = false, table = true;
  TableView<T> phi, g;                    // the handle's pair table; the radial tables, slot t_i ntypes + t_j
  const TableKnot<T>* __restrict__ ang;   // [ntypes^3] F := Lambda, U := cos0 of [t_i][t_j][t_k], in global memory
  __device__ __forceinline__ int32_t row(int32_t row, int32_t) const { return phi.type(row); }
  __device__ __forceinline__ const TableKnot<T>* entry(int32_t tp, int32_t j) const { return phi.slot(tp, j); }
  __device__ __forceinline__ void pair(const TableKnot<T>* slot, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    const T r2 = dx * dx + dy * dy + dz * dz;
    const bool inp = r2 < phi.xc && r2 > (T)0;
    const T s = (r2 - phi.x0) * phi.iD;
    const bool below = r2 < phi.x0;
    const int32_t k = inp && !below ? min((int32_t)s, phi.nknots - 2) : 0;
    const TableKnot<T> w = slot[k];
    const T t = s - (T)k;
    const T fr = inp ? (below ? (T)NAN : w.F + t * w.dF) : (T)0;
    pe = inp ? (below ? (T)NAN : w.U + t * w.dU) : (T)0;
    fx = fr * dx, fy = fr * dy, fz = fr * dz;
    in = inp || (r2 < g.xc && r2 > (T)0);
  }
};

// A wave's strip: the compacted in_3 partners of the row it is at, {j, a_x, a_y, a_z} of 64 slots, one array each.
template <typename T> struct SwStrip {
  int32_t* j;
  T *x, *y, *z;
};
template <typename T> constexpr size_t sw_strip_bytes() { return (size_t)WAVE * (3 * sizeof(T) + 4); }  // (a wave's)
// the strips of a block lie at 16-byte word `at16` of its dynamic LDS: behind the staged tables, or at its start
template <typename T> __device__ __forceinline__ SwStrip<T> sw_strip(int32_t at16) {
  extern __shared__ uint4 table_lds[];
  char* base = reinterpret_cast<char*>(table_lds + at16) + (threadIdx.x >> 6) * sw_strip_bytes<T>();
  T* x = reinterpret_cast<T*>(base);
  return {reinterpret_cast<int32_t*>(x + 3 * WAVE), x, x + WAVE, x + 2 * WAVE};
}

template <typename T> __device__ __forceinline__ T readlane_t(T v, int32_t src) {
  if constexpr (sizeof(T) == 4) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
  } else {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
  }
}
template <typename T> __device__ __forceinline__ T sqrt_t(T v) {
  if constexpr (sizeof(T) == 4) return sqrtf(v);
  else return sqrt(v);
}

// What a lane holds of its end j of the row's triples once sw_row is through.  m: the in_3 partners of the row (uniform);
// live: this lane holds an end of a triple (lane < m, 2 <= m <= 64); F = sum over k of the force on j, e = sum over k of h.
template <typename T> struct SwEnd {
  int32_t m, j;
  bool live;
  T ax, ay, az, fx, fy, fz, e;
};

// Steps 1 to 3 of a row.  on_pair: what the kernel does with the pair part of an entry.
template <typename T, typename OFF, bool TRI, typename F>
__device__ __forceinline__ SwEnd<T> sw_row(const LjArgs<T, OFF>& a, const SwPair<T>& p, const SwStrip<T>& st, int32_t row, int32_t lane,
                                            F&& on_pair) {
  int32_t m = 0;
  lj_row_pairs<T, OFF, TRI>(a, p, row, lane, [&](int32_t j, LjPartner w, T dx, T dy, T dz, T fx, T fy, T fz, T pe, bool in) {
    on_pair(w, dx, dy, dz, fx, fy, fz, pe, in);
    const T r2 = dx * dx + dy * dy + dz * dz;
    const bool in3 = r2 < p.g.xc && r2 > (T)0;
    const uint64_t hit = __ballot(in3);  // (of the lanes still in the walk: the others hold no entry)
    const int32_t at = m + (int32_t)lanes_below(hit);
    if (in3 && at < WAVE) st.j[at] = j, st.x[at] = dx, st.y[at] = dy, st.z[at] = dz;
    m += (int32_t)__popcll(hit);
  });
  m = __builtin_amdgcn_readfirstlane(m);  // (lane 0 is in every chunk of the walk)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  SwEnd<T> o;
  o.m = m;
  o.live = m >= 2 && m <= WAVE && lane < m;  // (one partner forms no triple; more than 64 have no value)
  o.j = o.live ? st.j[lane] : row;
  o.ax = o.live ? st.x[lane] : (T)1, o.ay = o.live ? st.y[lane] : (T)0, o.az = o.live ? st.z[lane] : (T)0;
  __builtin_amdgcn_wave_barrier();  // (the next row's writes stay behind these reads)
  o.fx = o.fy = o.fz = o.e = (T)0;
  if (m < 2 || m > WAVE) return o;  // (uniform) no triple, or no value
  // step 2: this lane's partner
  const int32_t nt = p.g.ntypes;
  const int32_t ti = type_of(p.g.types, row, nt), tj = type_of(p.g.types, o.j, nt);
  const T r2 = o.ax * o.ax + o.ay * o.ay + o.az * o.az;
  const TableAt<T> at = p.g.knot(r2);
  const TableKnot<T> kn = (p.g.tab + (size_t)(ti * nt + tj) * p.g.nknots)[at.k];
  const T ga = at.below ? (T)NAN : kn.U + at.t * kn.dU, Ga = at.below ? (T)NAN : kn.F + at.t * kn.dF;
  const T ir = (T)1 / sqrt_t(r2);
  const T ir2 = ir * ir;
  const TableKnot<T>* __restrict__ an = p.ang + (size_t)(ti * nt + tj) * nt;
  const TableKnot<T> p0 = an[0], p1 = an[min(1, nt - 1)], p2 = an[min(2, nt - 1)], p3 = an[min(3, nt - 1)];
  // step 3: every partner k against this lane's
  T sa = 0, sbx = 0, sby = 0, sbz = 0, e = 0;
  for (int32_t k = 0; k < m; k++) {
    const T bx = readlane_t(o.ax, k), by = readlane_t(o.ay, k), bz = readlane_t(o.az, k);
    const T irb = readlane_t(ir, k), gb = readlane_t(ga, k);
    const int32_t tk = __builtin_amdgcn_readlane(tj, k);
    const T lam = tk == 0 ? p0.F : tk == 1 ? p1.F : tk == 2 ? p2.F : p3.F;
    const T c0 = tk == 0 ? p0.U : tk == 1 ? p1.U : tk == 2 ? p2.U : p3.U;
    const T cs = (((o.ax * bx + o.ay * by) + o.az * bz) * ir) * irb;
    const T dc = cs - c0;
    const T ld = lam * dc;
    const T ldd = ld * dc;
    const T q = ga * gb;
    const T h = ldd * q;
    const T a2 = (ld + ld) * q;
    const T cb = a2 * (ir * irb);
    const T ca = ldd * (Ga * gb) + a2 * (cs * ir2);
    const bool use = k != lane;
    e += use ? h : (T)0, sa += use ? ca : (T)0;
    sbx += use ? cb * bx : (T)0, sby += use ? cb * by : (T)0, sbz += use ? cb * bz : (T)0;
  }
  if (o.live) o.fx = sbx - sa * o.ax, o.fy = sby - sa * o.ay, o.fz = sbz - sa * o.az, o.e = e;
  return o;
}

// The forces of one row, f zeroed in front of the launch.  A list whose build failed (status) gives NaN.
template <typename T, typename OFF, bool TRI>
__device__ __forceinline__ void sw_forces_row(const LjArgs<T, OFF>& a, const SwPair<T>& p, const SwStrip<T>& st, T* __restrict__ f, int32_t row,
                                              int32_t lane) {
  const T nan = (T)NAN;
  if (a.status && *a.status != 0u) {  // (uniform: every row of the launch takes this branch, so no atomic meets the store)
    if (lane == 0) f[(size_t)row * 4 + 0] = nan, f[(size_t)row * 4 + 1] = nan, f[(size_t)row * 4 + 2] = nan, f[(size_t)row * 4 + 3] = nan;
    return;
  }
  T ax = 0, ay = 0, az = 0, ae = 0;
  const SwEnd<T> o = sw_row<T, OFF, TRI>(a, p, st, row, lane, [&](LjPartner, T, T, T, T fx, T fy, T fz, T pe, bool) {
    ax += fx, ay += fy, az += fz, ae += (T)0.5 * pe;
  });
  if (o.m > WAVE) {  // (uniform) more in-range partners than lanes: the centre and every one of them has no value
    lj_row_pairs<T, OFF, TRI>(a, p, row, lane, [&](int32_t j, LjPartner, T dx, T dy, T dz, T, T, T, T, bool) {
      const T r2 = dx * dx + dy * dy + dz * dz;
      if (r2 < p.g.xc && r2 > (T)0) {
        atomicAdd(&f[(size_t)j * 4 + 0], nan), atomicAdd(&f[(size_t)j * 4 + 1], nan);
        atomicAdd(&f[(size_t)j * 4 + 2], nan), atomicAdd(&f[(size_t)j * 4 + 3], nan);
      }
    });
    ax = ay = az = ae = nan;
  }
  ax = wave_sum(ax), ay = wave_sum(ay), az = wave_sum(az), ae = wave_sum(ae);
  const T cx = -wave_sum(o.fx), cy = -wave_sum(o.fy), cz = -wave_sum(o.fz), ce = wave_sum(o.e) * (T)(1.0 / 6.0);
  if (o.live) {
    atomicAdd(&f[(size_t)o.j * 4 + 0], o.fx), atomicAdd(&f[(size_t)o.j * 4 + 1], o.fy);
    atomicAdd(&f[(size_t)o.j * 4 + 2], o.fz), atomicAdd(&f[(size_t)o.j * 4 + 3], o.e * (T)(1.0 / 3.0));
  }
  if (lane == 0) {
    atomicAdd(&f[(size_t)row * 4 + 0], ax + cx), atomicAdd(&f[(size_t)row * 4 + 1], ay + cy);
    atomicAdd(&f[(size_t)row * 4 + 2], az + cz), atomicAdd(&f[(size_t)row * 4 + 3], ae + ce);
  }
}

// n16_phi, n16_g: the two tables in 16-byte words (LDS instances: the strips lie behind them).
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_sw_forces(LjArgs<T, OFF> a, SwPair<T> p, int32_t n16_phi, int32_t n16_g, T* __restrict__ f) {
  if constexpr (LDS) table_stage(p.phi, n16_phi, &p.g, n16_g);
  const SwStrip<T> st = sw_strip<T>(LDS ? n16_phi + n16_g : 0);
  grid_rows(a.n, [&](int32_t row, int32_t lane) { sw_forces_row<T, OFF, TRI>(a, p, st, f, row, lane); });
}

// The totals: lj_virial_rows' sums and tree with the three-body terms of every row behind its pair terms.
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_sw_virial(LjArgs<T, OFF> a, SwPair<T> p, int32_t n16_phi, int32_t n16_g,
                                                             double* __restrict__ part) {
  __shared__ double red[4][VIR_OUT];
  if constexpr (LDS) table_stage(p.phi, n16_phi, &p.g, n16_g);
  const SwStrip<T> st = sw_strip<T>(LDS ? n16_phi + n16_g : 0);
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[VIR_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool ok = !(a.status && *a.status != 0u);  // (uniform over the launch; a failed list: k_virial_reduce writes the NaN)
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; ok && row < a.n; row += (int32_t)gridDim.x * 4) {
    const SwEnd<T> o = sw_row<T, OFF, TRI>(a, p, st, row, lane, [&](LjPartner, T dx, T dy, T dz, T fx, T fy, T fz, T pe, bool in) {
      const T wxx = fx * dx, wyy = fy * dy, wzz = fz * dz, wxy = fx * dy, wxz = fx * dz, wyz = fy * dz;
      acc[0] += (double)wxx, acc[1] += (double)wyy, acc[2] += (double)wzz;
      acc[3] += (double)wxy, acc[4] += (double)wxz, acc[5] += (double)wyz;
      acc[6] += (double)pe;
      acc[7] += in ? 1.0 : 0.0;
      acc[7] += (in && pe != pe) ? (double)NAN : 0.0;
    });
    if (o.m > WAVE) {
#pragma unroll
      for (int c = 0; c < VIR_OUT; c++) acc[c] += (double)NAN;
    }
    if (o.live) {  // W_cd -= a_c F_j,d, twice in front of the 1/2 of a full list; e_j holds every triple of the row twice over the lanes
      const T wxx = -(o.ax * o.fx), wyy = -(o.ay * o.fy), wzz = -(o.az * o.fz), wxy = -(o.ax * o.fy), wxz = -(o.ax * o.fz), wyz = -(o.ay * o.fz);
      acc[0] += 2.0 * (double)wxx, acc[1] += 2.0 * (double)wyy, acc[2] += 2.0 * (double)wzz;
      acc[3] += 2.0 * (double)wxy, acc[4] += 2.0 * (double)wxz, acc[5] += 2.0 * (double)wyz;
      acc[6] += (double)o.e;
      acc[7] += (o.e != o.e) ? (double)NAN : 0.0;
    }
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
size_t sw_strips_bytes(nl_handle_t h) { return 4 * (h->dtype == NL_F32 ? sw_strip_bytes<float>() : sw_strip_bytes<double>()); }
size_t sw_g_bytes(nl_handle_t h) { return table_bytes(h, h->sw); }
// the pair table, the g tables and the block's strips together
bool sw_in_lds(nl_handle_t h) { return table_in_lds(h->sw, sw_g_bytes(h) + table_bytes(h, h->tb) + sw_strips_bytes(h)); }

template <typename T> SwPair<T> sw_pair(nl_handle_t h) {
  const TableKnot<T>* ang = reinterpret_cast<const TableKnot<T>*>(static_cast<const char*>(h->sw.tab.get()) + sw_g_bytes(h));
  return {table_view<T>(h->tb, h->tb.tab, h->ty_types), table_view<T>(h->sw, h->sw.tab, h->ty_types), ang};
}

int sw_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, void* f_dev, hipStream_t s, const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bg = sw_g_bytes(h), bs = sw_strips_bytes(h);
  return rows_launch(h, q_dev, stride, f_dev, 4, s, status, [&](auto i, const auto& a, auto* f) {
    using I = decltype(i);
    using T = typename I::T;
    if constexpr (!I::half) {  // (sw_reach: full lists only)
      zero_async(f, 4 * (size_t)a.n, s);
      with_flag(sw_in_lds(h), [&](auto lds) {
        constexpr bool L = decltype(lds)::value;
        hipLaunchKernelGGL((k_sw_forces<T, typename I::OFF, I::tri, L>), dim3(table_blocks(a.n)), dim3(STAGE_THREADS), (L ? bp + bg : 0) + bs, s, a,
                           sw_pair<T>(h), (int32_t)(bp / 16), (int32_t)(bg / 16), f);
      });
    }
  });
}

int sw_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, double* out_dev, hipStream_t s, const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bg = sw_g_bytes(h), bs = sw_strips_bytes(h);
  return totals_launch(h, q_dev, stride, out_dev, s, status, NL_TABLE_BLOCKS, [&](auto i, const auto& a, int32_t nblk, double* part) {
    using I = decltype(i);
    using T = typename I::T;
    with_flag(sw_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_sw_virial<T, typename I::OFF, I::tri, L>), dim3(nblk), dim3(STAGE_THREADS), (L ? bp + bg : 0) + bs, s, a, sw_pair<T>(h),
                         (int32_t)(bp / 16), (int32_t)(bg / 16), part);
    });
    return NL_OK;
  });
}

// The pair table's conditions, then the three-body part's own: a whole single-device FULL list (a row must hold all partners of
// its centre, and the force on an owned end needs the triples centred on ghosts: slab lists are refused, local-index ones
// included) under what table_set_reach asks for the g tables.
int sw_reach(nl_handle_t h, double skin) {
  if (h->sw.nknots == 0) return fail(h, NL_ERR_STATE);
  if (int rc = table_reach(h, skin)) return rc;
  if (!h->plan.full || h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  return table_set_reach(h, h->sw, skin);
}

}  // namespace

extern "C" {

int nl_set_sw(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min_3, double r_max_3, const double* g_host, const double* G_host,
              const double* lambda_host, const double* cos0_host) {
  if (!h) return NL_ERR_ARG;
  if (nknots == 0 || (!g_host && !G_host && !lambda_host && !cos0_host)) {  // clear (the buffer stays, as the pair table's)
    h->sw.nknots = 0, h->sw.ntypes = 0;
    return NL_OK;
  }
  if (!g_host || !G_host || !lambda_host || !cos0_host || nknots < 2 || nknots > NL_TABLE_MAX_KNOTS || ntypes < 1 || ntypes > NL_SW_MAX_TYPES ||
      !(r_min_3 > 0) || !(r_min_3 < r_max_3) || !std::isfinite(r_max_3))
    return fail(h, NL_ERR_ARG);
  for (int32_t a = 0; a < ntypes; a++)
    for (int32_t b = 0; b < ntypes; b++)
      for (int32_t c = 0; c < ntypes; c++) {
        const int32_t at = (a * ntypes + b) * ntypes + c, ta = (a * ntypes + c) * ntypes + b;
        if (!std::isfinite(lambda_host[at]) || !(cos0_host[at] >= -1.0 && cos0_host[at] <= 1.0) || lambda_host[at] != lambda_host[ta] ||
            cos0_host[at] != cos0_host[ta])
          return fail(h, NL_ERR_ARG);
      }
  // the angular parameters ride behind the knots as one more segment: {Lambda, (difference), cos0, (difference)} per triple
  const TableSeg seg[2] = {{ntypes * ntypes, nknots, G_host, g_host}, {1, ntypes * ntypes * ntypes, lambda_host, cos0_host}};
  return table_upload(h, h->sw, ntypes, r_min_3, r_max_3, seg, 2);
}

int nl_get_sw(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min_3, double* r_max_3, int32_t* lds) {
  if (!h) return NL_ERR_ARG;
  if (h->sw.nknots == 0) return fail(h, NL_ERR_STATE);
  if (ntypes) *ntypes = h->sw.ntypes;
  if (nknots) *nknots = h->sw.nknots;
  if (r_min_3) *r_min_3 = h->sw.r_min;
  if (r_max_3) *r_max_3 = h->sw.r_max;
  if (lds) *lds = h->tb.nknots != 0 && sw_in_lds(h) ? 1 : 0;
  return NL_OK;
}

int nl_sw_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, false, sw_forces_launch, sw_reach);
}
int nl_sw_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, true, sw_forces_launch, sw_reach);
}
int nl_sw_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, false, sw_virial_launch, sw_reach);
}
int nl_sw_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, true, sw_virial_launch, sw_reach);
}

}  // extern "C"
