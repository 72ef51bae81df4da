// nl_tersoff.inc -- Tersoff-type bond-order potentials (DESIGN.md section 8y): E = sum_pairs phi(r) + sum_i sum_{j != i}
// 1/2 b(zeta_ij) u(r_ij), zeta_ij = p(r_ij) sum_{k != i, j} g(cos theta_jik) q(r_ik), from the full list of the last build.  The
// rule is stated at nl_set_tersoff in include/nl_hip.h.  Stillinger-Weber's row (nl_sw.inc) with a second pass over the partners,
// because the force needs b'(zeta_ij), which is known only after the whole sum over k.  One wave per centre row
//   1. walks the row with lj_row_pairs and TfPair (the pair table's arithmetic; in = in_phi || in_3) and compacts the in_3
//      partners {j, a} into the wave's LDS strip, as sw_row does;
//   2. lanes 0 .. m - 1 take a partner each: ir, and the knots of u, q and (where set) p of the slot (t_i, t_j) at one knot index
//      (the three tables share a grid);
//   3. loops k = 0 .. m - 1 (lane k's {b, ir_b, q_k, t_k} broadcast with v_readlane): S_j = sum_k g_jk q_k; then zeta_j, the two
//      pow of the bond order, b_j, b'_j, e_j = b_j u_j, w_j = (u_j / 2) b'_j, once per lane;
//   4. loops k again, w_k p_k broadcast as well: sa += ca, sb += cb b for k != j -- every lane keeps only its own end, no two
//      lanes add to one accumulator; F_j = sb - (sa + rad) a with the bond's own radial term rad;
//   5. writes out as nl_sw.inc step 4: F_j and e_j / 4 to f[j] by atomics, the row's own values (pair part - wave_sum(F_j); half
//      pair energy + wave_sum(e_j) / 4) by lane 0's atomics on the zeroed f; totals: -a_c F_j,d doubled (exact) and e_j into the
//      lane's double sums, no atomic, block partials for k_virial_reduce (whose 1/2 of a full list leaves e_j / 2 per bond).
// The angular parameters of (t_i, t_j, t_k) AND of (t_i, t_k, t_j) are needed per pass of the second loop: 32 values per lane
// for four types, 64 VGPRs in fp64.  They lie in a per-block LDS copy instead, {gamma, gc, d2, h} per triple of types and
// {beta, n, e2, 0} per pair of types behind them (at most 80 entries of 4 T), in front of the strips: two 16-byte reads per pass
// in fp32, all lanes of one type reading one address.
// m > NL_TERSOFF_MAX_NEAR: NaN to the centre, its in_3 partners (one more walk) and all 8 totals.
// The pieces are those of nl_table.inc, nl_consumer.inc and nl_sw.inc: TableView, table_stage, TableSet, table_upload,
// table_set_reach, grid_rows, table_blocks, rows_launch, totals_launch, pair_call, SwStrip, sw_strip, readlane_t.
// Included at the end of nl_api.hip, behind nl_sw.inc.

namespace {

static_assert(NL_TERSOFF_MAX_NEAR == WAVE, "one in-range partner per lane");
static_assert(NL_TERSOFF_MAX_TYPES == 4, "the LDS copy of the parameters holds 4^3 + 4^2 entries at most");

// The pair function of the walk: TableByPair's text on the pair table, and in = in_phi || in_3 for the pair count.
template <typename T> struct TfPair {
  static constexpr bool lanes_meet = false, table = true;
  TableView<T> phi, g;                    // the handle's pair table; the u tables, slot t_i ntypes + t_j (q, p behind them)
  const TableKnot<T>* __restrict__ par;   // global: [nt^3] {gamma, -, gc, -}, [nt^3] {d2, -, h, -}, [nt^2] {beta, -, n, -}, [nt^2] {e2, ..}
  int32_t has_p;                          // the p tables are set (uniform)
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

// An entry of the block's LDS copy of the parameters: {gamma, gc, d2, h} of a triple of types, {beta, n, e2, 0} of a pair.
template <typename T> struct alignas(16) TfParam {
  T a, b, c, d;
};
constexpr int32_t tf_params(int32_t nt) { return nt * nt * nt + nt * nt; }
template <typename T> constexpr size_t tf_param_bytes(int32_t nt) { return (size_t)tf_params(nt) * sizeof(TfParam<T>); }

// The parameters into the block's dynamic LDS at 16-byte word at16; no barrier (the caller's table_stage or __syncthreads).
template <typename T> __device__ __forceinline__ const TfParam<T>* tf_stage_params(const TfPair<T>& p, int32_t at16) {
  extern __shared__ uint4 table_lds[];
  TfParam<T>* out = reinterpret_cast<TfParam<T>*>(table_lds + at16);
  const int32_t nt = p.g.ntypes, n3 = nt * nt * nt, n2 = nt * nt;
  for (int32_t t = threadIdx.x; t < n3 + n2; t += STAGE_THREADS) {
    if (t < n3) out[t] = {p.par[t].F, p.par[t].U, p.par[n3 + t].F, p.par[n3 + t].U};
    else out[t] = {p.par[2 * n3 + (t - n3)].F, p.par[2 * n3 + (t - n3)].U, p.par[2 * n3 + n2 + (t - n3)].F, (T)0};
  }
  return out;
}

template <typename T> __device__ __forceinline__ T pow_t(T x, T y) {
  if constexpr (sizeof(T) == 4) return powf(x, y);
  else return pow(x, y);
}

// What a lane holds of its end j of the row's bonds once tf_row is through.  m: the in_3 partners of the row (uniform); live:
// this lane holds a bond (lane < m, 1 <= m <= 64); F: the force on j from the bonds of this centre, e = b_j u_j.
template <typename T> struct TfEnd {
  int32_t m, j;
  bool live;
  T ax, ay, az, fx, fy, fz, e;
};

// Steps 1 to 4 of a row.  on_pair: what the kernel does with the pair part of an entry.
template <typename T, typename OFF, bool TRI, typename F>
__device__ __forceinline__ TfEnd<T> tf_row(const LjArgs<T, OFF>& a, const TfPair<T>& p, const TfParam<T>* par, const SwStrip<T>& st, int32_t row,
                                            int32_t lane, F&& on_pair) {
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
  TfEnd<T> o;
  o.m = m;
  o.live = m >= 1 && m <= WAVE && lane < m;  // (a lone partner still has its bond; more than 64 have no value)
  o.j = o.live ? st.j[lane] : row;
  o.ax = o.live ? st.x[lane] : (T)1, o.ay = o.live ? st.y[lane] : (T)0, o.az = o.live ? st.z[lane] : (T)0;
  __builtin_amdgcn_wave_barrier();  // (the next row's writes stay behind these reads)
  o.fx = o.fy = o.fz = o.e = (T)0;
  if (m < 1 || m > WAVE) return o;  // (uniform) no bond, or no value
  // step 2: this lane's partner
  const int32_t nt = p.g.ntypes, nk = p.g.nknots;
  const int32_t ti = type_of(p.g.types, row, nt), tj = type_of(p.g.types, o.j, nt);
  const T r2 = o.ax * o.ax + o.ay * o.ay + o.az * o.az;
  const TableAt<T> at = p.g.knot(r2);
  const TableKnot<T>* __restrict__ slot = p.g.tab + (size_t)(ti * nt + tj) * nk + at.k;
  const size_t tab = (size_t)nt * nt * nk;  // one table: u, behind it q, behind it p
  const TableKnot<T> ku = slot[0], kq = slot[tab];
  const T nan = (T)NAN;
  const T uj = at.below ? nan : ku.U + at.t * ku.dU, Uj = at.below ? nan : ku.F + at.t * ku.dF;
  const T qj = at.below ? nan : kq.U + at.t * kq.dU, Qj = at.below ? nan : kq.F + at.t * kq.dF;
  T pj = (T)1, Pj = (T)0;
  if (p.has_p) {  // (uniform)
    const TableKnot<T> kp = slot[2 * tab];
    pj = at.below ? nan : kp.U + at.t * kp.dU, Pj = at.below ? nan : kp.F + at.t * kp.dF;
  }
  const T ir = (T)1 / sqrt_t(r2);
  const TfParam<T>* __restrict__ ang = par + (ti * nt) * nt;  // [t_j][t_k] of this centre type
  const TfParam<T> bo = par[nt * nt * nt + ti * nt + tj];     // {beta, n, e2}
  // step 3: S_j
  T S = 0;
  for (int32_t k = 0; k < m; k++) {
    const T bx = readlane_t(o.ax, k), by = readlane_t(o.ay, k), bz = readlane_t(o.az, k);
    const T irb = readlane_t(ir, k), qk = readlane_t(qj, k);
    const int32_t tk = __builtin_amdgcn_readlane(tj, k);
    const TfParam<T> jk = ang[tj * nt + tk];
    const T cs = (((o.ax * bx + o.ay * by) + o.az * bz) * ir) * irb;
    const T x = jk.d - cs;
    const T x2 = x * x;
    const T den = jk.c + x2;
    const T g = jk.a + jk.b * (x2 / den);
    S += k != lane ? g * qk : (T)0;
  }
  const T zeta = pj * S;
  T b = (T)1, bp = (T)0;
  if (!(zeta <= (T)0)) {  // (a NaN goes through the formula)
    const T t = bo.a * zeta;
    const T tn = pow_t(t, bo.b);
    const T one = (T)1 + tn;
    b = pow_t(one, bo.c);
    bp = (((T)(-0.5) * b) * (tn / one)) / zeta;
  }
  const T e = b * uj;
  const T w = ((T)0.5 * uj) * bp;
  const T wp = w * pj;
  const T rad = ((T)0.5 * b) * Uj + (w * Pj) * S;  // (in front of the loop: one value lives through it, not five)
  // step 4: the forces on this lane's end
  T sa = 0, sbx = 0, sby = 0, sbz = 0;
  for (int32_t k = 0; k < m; k++) {
    const T bx = readlane_t(o.ax, k), by = readlane_t(o.ay, k), bz = readlane_t(o.az, k);
    const T irb = readlane_t(ir, k), qk = readlane_t(qj, k), wpk = readlane_t(wp, k);
    const int32_t tk = __builtin_amdgcn_readlane(tj, k);
    const TfParam<T> jk = ang[tj * nt + tk], kj = ang[tk * nt + tj];
    const T cs = (((o.ax * bx + o.ay * by) + o.az * bz) * ir) * irb;
    const T x = jk.d - cs;
    const T den = jk.c + x * x;
    const T gpjk = -((((jk.b + jk.b) * jk.c) * x) / (den * den));
    const T y = kj.d - cs;
    const T y2 = y * y;
    const T dek = kj.c + y2;
    const T gkj = kj.a + kj.b * (y2 / dek);
    const T gpkj = -((((kj.b + kj.b) * kj.c) * y) / (dek * dek));
    const T cc = (wp * gpjk) * qk + (wpk * gpkj) * qj;
    const T cb = cc * (ir * irb);
    const T ca = cc * (cs * (ir * ir)) + (wpk * gkj) * Qj;  // (ir2_a again: a register less through the loop)
    const bool use = k != lane;
    sa += use ? ca : (T)0;
    sbx += use ? cb * bx : (T)0, sby += use ? cb * by : (T)0, sbz += use ? cb * bz : (T)0;
  }
  const T sat = sa + rad;
  if (o.live) o.fx = sbx - sat * o.ax, o.fy = sby - sat * o.ay, o.fz = sbz - sat * o.az, o.e = e;
  return o;
}

// The forces of one row, f zeroed in front of the launch.  A list whose build failed (status) gives NaN.
template <typename T, typename OFF, bool TRI>
__device__ __forceinline__ void tf_forces_row(const LjArgs<T, OFF>& a, const TfPair<T>& p, const TfParam<T>* par, const SwStrip<T>& st,
                                              T* __restrict__ f, int32_t row, int32_t lane) {
  const T nan = (T)NAN;
  if (a.status && *a.status != 0u) {  // (uniform: every row of the launch takes this branch, so no atomic meets the store)
    if (lane == 0) f[(size_t)row * 4 + 0] = nan, f[(size_t)row * 4 + 1] = nan, f[(size_t)row * 4 + 2] = nan, f[(size_t)row * 4 + 3] = nan;
    return;
  }
  T ax = 0, ay = 0, az = 0, ae = 0;
  const TfEnd<T> o = tf_row<T, OFF, TRI>(a, p, par, st, row, lane, [&](LjPartner, T, T, T, T fx, T fy, T fz, T pe, bool) {
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
  const T cx = -wave_sum(o.fx), cy = -wave_sum(o.fy), cz = -wave_sum(o.fz), ce = wave_sum(o.e) * (T)0.25;
  if (o.live) {
    atomicAdd(&f[(size_t)o.j * 4 + 0], o.fx), atomicAdd(&f[(size_t)o.j * 4 + 1], o.fy);
    atomicAdd(&f[(size_t)o.j * 4 + 2], o.fz), atomicAdd(&f[(size_t)o.j * 4 + 3], o.e * (T)0.25);
  }
  if (lane == 0) {
    atomicAdd(&f[(size_t)row * 4 + 0], ax + cx), atomicAdd(&f[(size_t)row * 4 + 1], ay + cy);
    atomicAdd(&f[(size_t)row * 4 + 2], az + cz), atomicAdd(&f[(size_t)row * 4 + 3], ae + ce);
  }
}

// The block's dynamic LDS: the staged tables (LDS instances), the parameters, the strips.  n16_phi, n16_g: the pair table and
// the radial tables (u, q and p together) in 16-byte words.
template <typename T, bool LDS> struct TfLds {
  const TfParam<T>* par;
  SwStrip<T> st;
  __device__ __forceinline__ TfLds(TfPair<T>& p, int32_t n16_phi, int32_t n16_g) {
    const int32_t at16 = LDS ? n16_phi + n16_g : 0;
    par = tf_stage_params(p, at16);
    if constexpr (LDS) table_stage(p.phi, n16_phi, &p.g, n16_g);
    else __syncthreads();
    st = sw_strip<T>(at16 + (int32_t)(tf_param_bytes<T>(p.g.ntypes) / 16));
  }
};

// fp32: 8 waves per SIMD (64 VGPRs), the occupancy of k_sw_forces; fp64: 4 (DESIGN.md section 8y has the table)
template <typename T> constexpr int tf_waves() { return sizeof(T) == 4 ? 8 : 4; }

template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS, tf_waves<T>()) k_tersoff_forces(LjArgs<T, OFF> a, TfPair<T> p, int32_t n16_phi, int32_t n16_g, T* __restrict__ f) {
  const TfLds<T, LDS> l(p, n16_phi, n16_g);
  grid_rows(a.n, [&](int32_t row, int32_t lane) { tf_forces_row<T, OFF, TRI>(a, p, l.par, l.st, f, row, lane); });
}

// The totals: lj_virial_rows' sums and tree with the bond terms of every row behind its pair terms.
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS, tf_waves<T>()) k_tersoff_virial(LjArgs<T, OFF> a, TfPair<T> p, int32_t n16_phi, int32_t n16_g,
                                                                  double* __restrict__ part) {
  __shared__ double red[4][VIR_OUT];
  const TfLds<T, LDS> l(p, n16_phi, n16_g);
  // (the wave in a scalar register, the thread from it and the lane at the end: held in vector registers through the rows they
  // are the three that would not fit the 64 of an fp32 instance)
  const int32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  double acc[VIR_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool ok = !(a.status && *a.status != 0u);  // (uniform over the launch; a failed list: k_virial_reduce writes the NaN)
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; ok && row < a.n; row += (int32_t)gridDim.x * 4) {
    const TfEnd<T> o = tf_row<T, OFF, TRI>(a, p, l.par, l.st, row, lane, [&](LjPartner, T dx, T dy, T dz, T fx, T fy, T fz, T pe, bool in) {
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
    if (o.live) {  // W_cd -= a_c F_j,d, twice in front of the 1/2 of a full list; e_j: that 1/2 leaves e_j / 2 of every ordered bond
      const T wxx = -(o.ax * o.fx), wyy = -(o.ay * o.fy), wzz = -(o.az * o.fz), wxy = -(o.ax * o.fy), wxz = -(o.ax * o.fz), wyz = -(o.ay * o.fz);
      acc[0] += 2.0 * (double)wxx, acc[1] += 2.0 * (double)wyy, acc[2] += 2.0 * (double)wzz;
      acc[3] += 2.0 * (double)wxy, acc[4] += 2.0 * (double)wxz, acc[5] += 2.0 * (double)wyz;
      acc[6] += (double)o.e;
      acc[7] += (o.e != o.e || o.fx != o.fx) ? (double)NAN : 0.0;
    }
  }
#pragma unroll
  for (int c = 0; c < VIR_OUT; c++) acc[c] = wave_sum(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < VIR_OUT; c++) red[wave][c] = acc[c];
  }
  __syncthreads();
  if (wave * WAVE + lane < VIR_OUT) {
    const int c = wave * WAVE + lane;
    part[(size_t)blockIdx.x * VIR_OUT + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  }
}

// ---- host side
size_t tf_radial_bytes(nl_handle_t h) { return table_bytes(h, h->tf) * (h->tf_p ? 3 : 2); }  // u, q and (where set) p
size_t tf_lds_tail_bytes(nl_handle_t h) {  // the parameters and the block's strips
  const bool f32 = h->dtype == NL_F32;
  return (f32 ? tf_param_bytes<float>(h->tf.ntypes) : tf_param_bytes<double>(h->tf.ntypes)) + sw_strips_bytes(h);
}
// the pair table, the radial tables, the parameters and the block's strips together
bool tf_in_lds(nl_handle_t h) { return table_in_lds(h->tf, tf_radial_bytes(h) + table_bytes(h, h->tb) + tf_lds_tail_bytes(h)); }

template <typename T> TfPair<T> tf_pair(nl_handle_t h) {
  const TableKnot<T>* par = reinterpret_cast<const TableKnot<T>*>(static_cast<const char*>(h->tf.tab.get()) + tf_radial_bytes(h));
  return {table_view<T>(h->tb, h->tb.tab, h->ty_types), table_view<T>(h->tf, h->tf.tab, h->ty_types), par, h->tf_p ? 1 : 0};
}

int tf_forces_launch(nl_handle_t h, const void* q_dev, int32_t stride, void* f_dev, hipStream_t s, const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bg = tf_radial_bytes(h), bs = tf_lds_tail_bytes(h);
  return rows_launch(h, q_dev, stride, f_dev, 4, s, status, [&](auto i, const auto& a, auto* f) {
    using I = decltype(i);
    using T = typename I::T;
    if constexpr (!I::half) {  // (tf_reach: full lists only)
      zero_async(f, 4 * (size_t)a.n, s);
      with_flag(tf_in_lds(h), [&](auto lds) {
        constexpr bool L = decltype(lds)::value;
        hipLaunchKernelGGL((k_tersoff_forces<T, typename I::OFF, I::tri, L>), dim3(table_blocks(a.n)), dim3(STAGE_THREADS), (L ? bp + bg : 0) + bs, s,
                           a, tf_pair<T>(h), (int32_t)(bp / 16), (int32_t)(bg / 16), f);
      });
    }
  });
}

int tf_virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, double* out_dev, hipStream_t s, const uint32_t* status) {
  const size_t bp = table_bytes(h, h->tb), bg = tf_radial_bytes(h), bs = tf_lds_tail_bytes(h);
  return totals_launch(h, q_dev, stride, out_dev, s, status, NL_TABLE_BLOCKS, [&](auto i, const auto& a, int32_t nblk, double* part) {
    using I = decltype(i);
    using T = typename I::T;
    with_flag(tf_in_lds(h), [&](auto lds) {
      constexpr bool L = decltype(lds)::value;
      hipLaunchKernelGGL((k_tersoff_virial<T, typename I::OFF, I::tri, L>), dim3(nblk), dim3(STAGE_THREADS), (L ? bp + bg : 0) + bs, s, a,
                         tf_pair<T>(h), (int32_t)(bp / 16), (int32_t)(bg / 16), part);
    });
    return NL_OK;
  });
}

// sw_reach's conditions on the Tersoff set: the pair table's, a whole single-device FULL list, the reach of the radial tables.
int tf_reach(nl_handle_t h, double skin) {
  if (h->tf.nknots == 0) return fail(h, NL_ERR_STATE);
  if (int rc = table_reach(h, skin)) return rc;
  if (!h->plan.full || h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  return table_set_reach(h, h->tf, skin);
}

}  // namespace

extern "C" {

int nl_set_tersoff(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min_3, double r_max_3, const double* u_host, const double* U_host,
                   const double* q_host, const double* Q_host, const double* p_host, const double* P_host, const double* gamma_host,
                   const double* c2_over_d2_host, const double* d2_host, const double* h_host, const double* beta_host, const double* n_host) {
  if (!h) return NL_ERR_ARG;
  const double* need[] = {u_host, U_host, q_host, Q_host, gamma_host, c2_over_d2_host, d2_host, h_host, beta_host, n_host};
  bool all = true, none = !p_host && !P_host;
  for (const double* v : need) all = all && v, none = none && !v;
  if (nknots == 0 || none) {  // clear (the buffer stays, as the pair table's)
    h->tf.nknots = 0, h->tf.ntypes = 0;
    return NL_OK;
  }
  if (!all || !p_host != !P_host || nknots < 2 || nknots > NL_TABLE_MAX_KNOTS || ntypes < 1 || ntypes > NL_TERSOFF_MAX_TYPES || !(r_min_3 > 0) ||
      !(r_min_3 < r_max_3) || !std::isfinite(r_max_3))
    return fail(h, NL_ERR_ARG);
  const int32_t n2 = ntypes * ntypes, n3 = n2 * ntypes;
  std::vector<double> gc(n3), e2(n2);
  for (int32_t t = 0; t < n3; t++) {
    if (!std::isfinite(gamma_host[t]) || !std::isfinite(c2_over_d2_host[t]) || !std::isfinite(h_host[t]) || !std::isfinite(d2_host[t]) ||
        !(d2_host[t] > 0))
      return fail(h, NL_ERR_ARG);
    gc[t] = gamma_host[t] * c2_over_d2_host[t];
  }
  for (int32_t t = 0; t < n2; t++) {
    if (!std::isfinite(beta_host[t]) || !(beta_host[t] >= 0) || !std::isfinite(n_host[t]) || !(n_host[t] > 0)) return fail(h, NL_ERR_ARG);
    e2[t] = -1.0 / (2.0 * n_host[t]);
  }
  // behind the knots ride the parameters as four more segments (table_upload checks that gc and e2 are finite as well)
  TableSeg seg[7];
  int ns = 0;
  seg[ns++] = {n2, nknots, U_host, u_host};
  seg[ns++] = {n2, nknots, Q_host, q_host};
  if (p_host) seg[ns++] = {n2, nknots, P_host, p_host};
  seg[ns++] = {1, n3, gamma_host, gc.data()};
  seg[ns++] = {1, n3, d2_host, h_host};
  seg[ns++] = {1, n2, beta_host, n_host};
  seg[ns++] = {1, n2, e2.data(), e2.data()};
  const int rc = table_upload(h, h->tf, ntypes, r_min_3, r_max_3, seg, ns);
  if (rc == NL_OK) h->tf_p = p_host != nullptr;
  return rc;
}

int nl_get_tersoff(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min_3, double* r_max_3, int32_t* has_p, int32_t* lds) {
  if (!h) return NL_ERR_ARG;
  if (h->tf.nknots == 0) return fail(h, NL_ERR_STATE);
  if (ntypes) *ntypes = h->tf.ntypes;
  if (nknots) *nknots = h->tf.nknots;
  if (r_min_3) *r_min_3 = h->tf.r_min;
  if (r_max_3) *r_max_3 = h->tf.r_max;
  if (has_p) *has_p = h->tf_p ? 1 : 0;
  if (lds) *lds = h->tb.nknots != 0 && tf_in_lds(h) ? 1 : 0;
  return NL_OK;
}

int nl_tersoff_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, false, tf_forces_launch, tf_reach);
}
int nl_tersoff_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, f_dev, stream, true, tf_forces_launch, tf_reach);
}
int nl_tersoff_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, false, tf_virial_launch, tf_reach);
}
int nl_tersoff_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return pair_call(h, q_dev, q_stride, out_dev, stream, true, tf_virial_launch, tf_reach);
}

}  // extern "C"
