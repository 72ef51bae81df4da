// nl_consumer.inc -- a consumer of the list (SURVEY.md section 8 f3): truncated Lennard-Jones forces and per-particle
// potential energy from the CSR of the last build.  Absent in the reference (it allocates a momentum array and never
// uses it, make_list.cpp:135,138-140); here it answers which list kind the builder should be optimised for.
//   full list: row i gathers its partners and writes f[i] once -- no atomics, every pair evaluated twice;
//   half list: every pair once, the reaction goes to f[j] with floating-point atomics.
// nl_lj_forces takes one epsilon, sigma and rc_force; nl_lj_forces_typed takes them per pair of types (nl_types.inc sets the
// tables).  One kernel body (lj_row) and one launch serve both.
// What the consumers of the list share is written once, here (DESIGN.md sections 8l, 8q): the arguments of a launch (LjArgs,
// lj_args), the walk of a row up to the pair's values (lj_row_pairs over lj_image and lj_pair), the rows of a persistent grid
// (grid_rows), a particle's type and a pair's slot (type_of, pair_slot), the launch of a kernel family over the rows
// (rows_launch; totals_launch in nl_virial.inc), first-call scratch, what the list guarantees (list_reach) and what an entry
// point does before its launch (consumer_call; lj_call and pair_call over it).  Included at the end of nl_api.hip.

namespace {

template <typename T> __device__ __forceinline__ void lj_pair(T dx, T dy, T dz, T eps4, T sig2, T rcf2, T& fx, T& fy, T& fz, T& pe, bool& in) {
  const T r2 = dx * dx + dy * dy + dz * dz;
  in = r2 < rcf2 && r2 > (T)0;
  const T ir2 = in ? sig2 / r2 : (T)0;
  const T s6 = ir2 * ir2 * ir2;
  // U = 4 eps (s12 - s6);  F = 24 eps (2 s12 - s6) / r^2 * d   (d = r_i - r_j, force on i)
  const T fr = in ? (T)6 * eps4 * (s6 + s6 - (T)1) * s6 / r2 : (T)0;
  fx = fr * dx, fy = fr * dy, fz = fr * dz;
  pe = eps4 * (s6 - (T)1) * s6;
}

// The image of a pair of the list's build: d = r_i - r_j folded on the periodic axes (L > 0; 0 = open axis) in z, y, x order,
// k_z = rint(dz / Lz), k_y = rint((dy - k_z yz) / Ly), k_x = rint((dx - k_z xz - k_y xy) / Lx) -- the rule of the skin check,
// in T.  Positions may lie up to one box length outside the box, as for the builds (drifted and never re-wrapped: nl_update_list
// with nl_set_pair_images), so a raw separation reaches +-3 L: one half-box test per axis is not enough, and neither is the
// rounded raw separation, whose error (half an ulp of 3 L) would make the forces depend on the image the caller's coordinates
// sit in.  So the separation is taken with its rounding error (two_diff: d + lo = r_i - r_j exactly), the lattice vector is
// taken off d with fma, the largest term first (exact for k L: the result is a multiple of ulp(L) below L / 2), and lo is added
// to the small result.  With a tilt a step can leave more than it found (dy = 3, k_z yz = -8.3: k_y = 1 and dy - Ly = -15.1, coarser
// than dy's own grid), so there every term of y and x goes through sub_kl, which keeps the step's rounding error in lo as well;
// z has no tilt and stays on the fma.  Every component of the image within rc is below L_d / 3 (mesh >= 3), so d / L is never near a
// half-integer: the reciprocal (loop-invariant) picks the same k, and this is the image the list used.
template <typename T> __device__ __forceinline__ T rint_t(T v) {
  if constexpr (sizeof(T) == 4) return rintf(v);
  else return rint(v);
}
template <typename T> __device__ __forceinline__ T fma_t(T a, T b, T c) {
  if constexpr (sizeof(T) == 4) return fmaf(a, b, c);
  else return fma(a, b, c);
}
template <typename T> __device__ __forceinline__ T two_diff(T a, T b, T& lo) {
  const T d = a - b, bv = d - a;
  lo = (a - (d - bv)) - (b + bv);
  return d;
}
// d + lo -= k m, exactly up to the rounding of lo (k m = p + pe and d - p = d' + e, both without error)
template <typename T> __device__ __forceinline__ void sub_kl(T k, T m, T& d, T& lo) {
  const T p = k * m, pe = fma_t(k, m, -p);
  T e;
  d = two_diff(d, p, e);
  lo += e - pe;
}
template <typename T, bool TRI>
__device__ __forceinline__ void lj_image(T xi, T yi, T zi, T xj, T yj, T zj, T& dx, T& dy, T& dz, T Lx, T Ly, T Lz, T xy, T xz,
                                         T yz) {
  if (!(Lx > (T)0 || Ly > (T)0 || Lz > (T)0)) {  // open box (uniform): the coordinates as given
    dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return;
  }
  T lx, ly, lz;
  dx = two_diff(xi, xj, lx), dy = two_diff(yi, yj, ly), dz = two_diff(zi, zj, lz);
  const T iLx = Lx > (T)0 ? (T)1 / Lx : (T)0, iLy = Ly > (T)0 ? (T)1 / Ly : (T)0, iLz = Lz > (T)0 ? (T)1 / Lz : (T)0;
  const T kz = rint_t(dz * iLz);
  T ty = dy, tx = dx;
  if constexpr (TRI) ty = ty - kz * yz, tx = tx - kz * xz;
  const T ky = rint_t(ty * iLy);
  if constexpr (TRI) tx = tx - ky * xy;
  const T kx = rint_t(tx * iLx);
  dz = fma_t(-kz, Lz, dz);
  if constexpr (TRI) {
    sub_kl(ky, Ly, dy, ly), sub_kl(kz, yz, dy, ly);
    sub_kl(kx, Lx, dx, lx), sub_kl(ky, xy, dx, lx), sub_kl(kz, xz, dx, lx);
  } else {
    dy = fma_t(-ky, Ly, dy);
    dx = fma_t(-kx, Lx, dx);
  }
  dx += lx, dy += ly, dz += lz;
}

// Where a pair's values come from -- the pair function is a property of PAR (DESIGN.md section 8o):
//   row(row, lane)    what a lane keeps for the whole row,
//   entry(r, j)       what the entry with partner j takes of it (lanes_meet: called by every lane of the wave, in step),
//   pair(e, d, ...)   the pair's values fx, fy, fz, pe, in from the separation.
// Lennard-Jones from the launch's scalars, or from a table over the types of the pair (nl_set_lj_type_params): lane
// t < ntypes holds eps4, sig2 and rcf2 of (t_row, t), an entry picks them by its partner's type with ds_bpermute.
// A tabulated potential: TableByPair of nl_table.inc.  table: the pair function may give NaN inside its range (a pair below
// the table), which the totals of nl_virial.inc carry into the pair count as well.
template <typename T> struct LjRow {
  T eps4, sig2, rcf2;
};
template <typename T> struct LjScalars {
  static constexpr bool lanes_meet = false, table = false;
  T eps4, sig2, rcf2;
  __device__ __forceinline__ LjRow<T> row(int32_t, int32_t) const { return {eps4, sig2, rcf2}; }
  __device__ __forceinline__ LjRow<T> entry(const LjRow<T>& r, int32_t) const { return r; }
  __device__ __forceinline__ void pair(const LjRow<T>& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    lj_pair<T>(dx, dy, dz, e.eps4, e.sig2, e.rcf2, fx, fy, fz, pe, in);
  }
};
template <typename T> struct LjByType {
  static constexpr bool lanes_meet = true, table = false;
  const int32_t* __restrict__ types;
  const T* __restrict__ par;  // [3][NL_MAX_TYPES][NL_MAX_TYPES] 4 eps, sigma^2, rc_force^2
  __device__ __forceinline__ LjRow<T> row(int32_t row, int32_t lane) const {  // this lane's entries of the row's type
    constexpr int NT2 = NL_MAX_TYPES * NL_MAX_TYPES;
    const int32_t at = (types[row] & (NL_MAX_TYPES - 1)) * NL_MAX_TYPES + (lane & (NL_MAX_TYPES - 1));
    return {par[at], par[NT2 + at], par[2 * NT2 + at]};
  }
  __device__ __forceinline__ LjRow<T> entry(const LjRow<T>& r, int32_t j) const {
    const int32_t tj = types[j] & (NL_MAX_TYPES - 1);
    return {shfl_t(r.eps4, tj), shfl_t(r.sig2, tj), shfl_t(r.rcf2, tj)};
  }
  __device__ __forceinline__ void pair(const LjRow<T>& e, T dx, T dy, T dz, T& fx, T& fy, T& fz, T& pe, bool& in) const {
    lj_pair<T>(dx, dy, dz, e.eps4, e.sig2, e.rcf2, fx, fy, fz, pe, in);
  }
};

// What every kernel over the pairs of the list receives (k_lj*, k_lj_virial*).  status (the enqueue variants, which do not
// wait for the build): the build's status word, nullptr otherwise.
template <typename T, typename OFF> struct LjArgs {
  const T* __restrict__ q;
  int32_t stride;
  const OFF* __restrict__ kp;
  const int32_t* __restrict__ list;
  int32_t n;  // rows of the list: the build's n_rows (a local-id slab build: ids from n on are ghosts, LjPartner)
  const uint32_t* __restrict__ status;
  T Lx, Ly, Lz, xy, xz, yz;
};

// What a row knows of an entry's partner besides its position (DESIGN.md section 8n).  ghost: j is no row of this list -- a
// ghost of a local-id slab build (nl_set_local_ids: owned rows first, j >= n_rows), whose owner stores the same pair in its own
// row; never set after a whole build, whose every id is a row.  first: of the two ranks that store an owned-ghost pair, this
// is the one that counts it -- dz < 0, or dz == 0 and z_i < z_j as given.  lj_image is odd under the swap of the two particles
// (two_diff, rint and fma are), so exactly one of the two rows says so.
struct LjPartner {
  bool ghost, first;
};

// The pairs of one row, a wave per row: on_pair(j, partner, dx, dy, dz, fx, fy, fz, pe, in) for every entry of the row, with
// the separation at the image the list found the pair at (minimum-image list, nl_set_periodic_axes: folded on the periodic
// axes, L > 0), the values of PAR's pair function and what LjPartner says of j.  a.n: the rows of the list (n_rows of the build).
template <typename T, typename OFF, bool TRI, typename PAR, typename F>
__device__ __forceinline__ void lj_row_pairs(const LjArgs<T, OFF>& a, const PAR& p, int32_t row, int32_t lane, F&& on_pair) {
  const auto rp = p.row(row, lane);
  T xi, yi, zi;
  load_xyz(a.q, a.stride, row, xi, yi, zi);
  const OFF b = a.kp[row], e = a.kp[row + 1];
  for (OFF k = b + lane; (PAR::lanes_meet ? k - lane : k) < e; k += 64) {  // (lanes_meet: every lane stays for the bpermute)
    const bool valid = !PAR::lanes_meet || k < e;
    const int32_t j = valid ? a.list[k] : row;
    const auto ep = p.entry(rp, j);
    if constexpr (PAR::lanes_meet) {
      if (!valid) continue;
    }
    T xj, yj, zj;
    load_xyz(a.q, a.stride, j, xj, yj, zj);
    T dx, dy, dz, fx, fy, fz, pe;
    bool in;
    lj_image<T, TRI>(xi, yi, zi, xj, yj, zj, dx, dy, dz, a.Lx, a.Ly, a.Lz, a.xy, a.xz, a.yz);
    p.pair(ep, dx, dy, dz, fx, fy, fz, pe, in);
    const LjPartner w = {j >= a.n, dz < (T)0 || (dz == (T)0 && zi < zj)};
    on_pair(j, w, dx, dy, dz, fx, fy, fz, pe, in);
  }
}

// one wave per row; f = {fx, fy, fz, pe_i} of the list's rows, pe_i = half of the pair energies of particle i.  A list whose
// build failed (status) gives NaN forces.
template <typename T, bool HALF, typename OFF, bool TRI, typename PAR>
__device__ __forceinline__ void lj_row_at(const LjArgs<T, OFF>& a, const PAR& p, T* __restrict__ f, int32_t row, int32_t lane) {
  if (a.status && *a.status != 0u) {  // (uniform: every row of the launch takes this branch)
    if (lane == 0) {
      const T nan = (T)NAN;
      f[(size_t)row * 4 + 0] = nan, f[(size_t)row * 4 + 1] = nan, f[(size_t)row * 4 + 2] = nan, f[(size_t)row * 4 + 3] = nan;
    }
    return;
  }
  T ax = 0, ay = 0, az = 0, ae = 0;
  lj_row_pairs<T, OFF, TRI>(a, p, row, lane, [&](int32_t j, LjPartner w, T, T, T, T fx, T fy, T fz, T pe, bool in) {
    ax += fx, ay += fy, az += fz, ae += (T)0.5 * pe;
    if (HALF && in && !w.ghost) {  // Newton's third law: the partner's share (a ghost gets its own from its owner's row)
      atomicAdd(&f[(size_t)j * 4 + 0], -fx);
      atomicAdd(&f[(size_t)j * 4 + 1], -fy);
      atomicAdd(&f[(size_t)j * 4 + 2], -fz);
      atomicAdd(&f[(size_t)j * 4 + 3], (T)0.5 * pe);
    }
  });
  ax = wave_sum(ax), ay = wave_sum(ay), az = wave_sum(az), ae = wave_sum(ae);
  if (lane == 0) {
    if (HALF) {
      atomicAdd(&f[(size_t)row * 4 + 0], ax);
      atomicAdd(&f[(size_t)row * 4 + 1], ay);
      atomicAdd(&f[(size_t)row * 4 + 2], az);
      atomicAdd(&f[(size_t)row * 4 + 3], ae);
    } else {
      f[(size_t)row * 4 + 0] = ax, f[(size_t)row * 4 + 1] = ay, f[(size_t)row * 4 + 2] = az, f[(size_t)row * 4 + 3] = ae;
    }
  }
}

// one block per 4 rows (k_lj*); the persistent grids walk lj_row_at themselves (grid_rows)
template <typename T, bool HALF, typename OFF, bool TRI, typename PAR>
__device__ __forceinline__ void lj_row(const LjArgs<T, OFF>& a, const PAR& p, T* __restrict__ f) {
  const int32_t row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= a.n) return;
  lj_row_at<T, HALF, OFF, TRI>(a, p, f, row, lane);
}

// The rows of a persistent grid of 4-wave blocks (the totals, the histogram, the tabulated and the EAM kernels): wave w of
// block b takes the rows 4 b + w, + 4 gridDim, ... below n; on_row(row, lane).
template <typename F> __device__ __forceinline__ void grid_rows(int32_t n, F&& on_row) {
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; row < n; row += (int32_t)gridDim.x * 4) on_row(row, lane);
}

// A particle's type as an index below ntypes (types == nullptr: everybody is type 0), and the triangular slot of an
// unordered pair of types (slot(a, b) of nl_pair_histogram_typed).  k_type_check: types < ntypes; the min keeps the slot
// inside its table whatever the type table holds.
__device__ __forceinline__ int32_t type_of(const int32_t* types, int32_t i, int32_t ntypes) {
  return types ? min(types[i] & (NL_MAX_TYPES - 1), ntypes - 1) : 0;
}
__device__ __forceinline__ int32_t pair_slot(int32_t ti, int32_t tj, int32_t ntypes) {
  const int32_t lo = min(ti, tj), hi = max(ti, tj);
  return lo * (2 * ntypes - lo + 1) / 2 + (hi - lo);
}

template <typename T, bool HALF, typename OFF, bool TRI>
__global__ void __launch_bounds__(256) k_lj(LjArgs<T, OFF> a, LjScalars<T> p, T* __restrict__ f) {
  lj_row<T, HALF, OFF, TRI>(a, p, f);
}
template <typename T, bool HALF, typename OFF, bool TRI>
__global__ void __launch_bounds__(256) k_lj_typed(LjArgs<T, OFF> a, LjByType<T> p, T* __restrict__ f) {
  lj_row<T, HALF, OFF, TRI>(a, p, f);
}

// Zeroes what a half list's atomics add to.  A kernel, not hipMemsetAsync: captured into a graph behind other work
// on the buffer (torch.cuda.graph; a fill of f in front of the replay), the memset node zeroed only some of every four words
// from the second replay on -- with the parent's library as with this one, eagerly never -- and the forces kept what was there.
template <typename T> __global__ void __launch_bounds__(256) k_lj_zero(T* __restrict__ f, size_t count) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) f[i] = (T)0;
}
template <typename T> void zero_async(T* ptr, size_t count, hipStream_t s) {
  hipLaunchKernelGGL((k_lj_zero<T>), dim3((unsigned)std::min<size_t>((count + 255) / 256, 8192)), dim3(256), 0, s, ptr, count);
}

// The arguments of a launch over the handle's list (rows_launch, totals_launch, hist_launch).  Box lengths for the minimum
// image on the axes of the list's build; 0 = open axis (the reference's distances, neighlist_cpu.hpp:219-223).  The box and
// the mask are the build's (BuildPlan::box, BuildPlan::pbc), not what nl_set_box or nl_set_periodic_axes may have set since;
// the launches take the triclinic instances where that box has a tilt (BuildPlan::tilt).
// lj_scalars, lj_by_type: the parameters of a launch, the scalars rounded to T once.
template <typename T, typename OFF> LjArgs<T, OFF> lj_args(nl_handle_t h, const void* q_dev, int32_t stride, const uint32_t* status) {
  const Box& b = h->plan.box;
  const int pbc = h->plan.pbc;
  return {static_cast<const T*>(q_dev), stride, static_cast<const OFF*>(h->key_pointer), h->list, h->n_rows, status,
          (pbc & 1) ? (T)b.L[0] : (T)0, (pbc & 2) ? (T)b.L[1] : (T)0, (pbc & 4) ? (T)b.L[2] : (T)0, (T)b.xy, (T)b.xz, (T)b.yz};
}
template <typename T> LjScalars<T> lj_scalars(const double* lj) { return {(T)(4.0 * lj[0]), (T)(lj[1] * lj[1]), (T)(lj[2] * lj[2])}; }
template <typename T> LjByType<T> lj_by_type(nl_handle_t h) { return {h->ty_types, static_cast<const T*>(h->lj_par)}; }

// The instance of a launch: the position and offset types of the build, half list, triclinic box.
template <typename T_, typename OFF_, bool HALF, bool TRI> struct Inst {
  using T = T_;
  using OFF = OFF_;
  static constexpr bool half = HALF, tri = TRI;
};

// A launch that leaves per_row values of T per row of the list in out_dev (forces: 4; the EAM densities: 1): nothing for an
// empty list; the arguments; zeroes in front of a half list's atomics; body(Inst, LjArgs, out) launches the family's kernels;
// the launch check.
template <typename BODY>
int rows_launch(nl_handle_t h, const void* q_dev, int32_t stride, void* out_dev, int32_t per_row, hipStream_t s, const uint32_t* status,
                BODY&& body) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    T* out = static_cast<T*>(out_dev);
    if (!h->plan.full) zero_async(out, (size_t)per_row * (size_t)n, s);
    with_flag(!h->plan.full, [&](auto half) {
      with_flag(h->plan.tilt, [&](auto tri) { body(Inst<T, OFF, decltype(half)::value, decltype(tri)::value>(), a, out); });
    });
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

// lj: {epsilon, sigma, rc_force} of the launch; nullptr: by type, from the handle's tables.
int lj_launch(nl_handle_t h, const void* q_dev, int32_t stride, const double* lj, void* f_dev, hipStream_t s, const uint32_t* status) {
  const int32_t nbw = (int32_t)(((int64_t)h->n_rows * 64 + 255) / 256);
  return rows_launch(h, q_dev, stride, f_dev, 4, s, status, [&](auto i, const auto& a, auto* f) {
    using I = decltype(i);
    using T = typename I::T;
    if (lj) hipLaunchKernelGGL((k_lj<T, I::half, typename I::OFF, I::tri>), dim3(nbw), dim3(256), 0, s, a, lj_scalars<T>(lj), f);
    else hipLaunchKernelGGL((k_lj_typed<T, I::half, typename I::OFF, I::tri>), dim3(nbw), dim3(256), 0, s, a, lj_by_type<T>(h), f);
  });
}

// First-call scratch of a consumer (vir_part, ea_part): allocated by the first call that needs it, which a stream that is
// being captured cannot do.
template <typename B> int first_call_scratch(nl_handle_t h, DevBuf<B>& b, size_t bytes, hipStream_t s) {
  if (b) return NL_OK;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIPCHK(h, hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) return fail(h, NL_ERR_STATE);
  return side_alloc(h, b, bytes);
}

// What the list guarantees: every pair within the smallest cut-off it was built with -- rc, and with a type table the rc_ab.
// skip_zero: a pair of types with rc_ab = 0 has no entries and asks for nothing (tables, typed histogram); otherwise it counts,
// and nothing is within it (untyped histogram).  A list that may be reused holds this less the skin.
double list_reach(nl_handle_t h, bool skip_zero) {
  double lim = h->rc;
  if (h->ty_types) {
    const int32_t nt = h->ty_ntypes;
    for (int32_t k = 0; k < nt * nt; k++)
      if (!skip_zero || h->ty_rc[k] > 0.0) lim = std::min(lim, h->ty_rc[k]);
  }
  return lim;
}

// The typed forces' preconditions beyond the untyped ones: a type table and parameters of its ntypes, and rc_force_ab
// within rc_ab (less the skin for the enqueue variant, whose list may be reused) -- pair of types by pair of types, which
// list_reach's one figure cannot say.
int lj_typed_check(nl_handle_t h, double skin) {
  if (!h->ty_types || !h->lj_par) return fail(h, NL_ERR_STATE);
  if (h->lj_ntypes != h->ty_ntypes) return fail(h, NL_ERR_ARG);
  const int32_t nt = h->ty_ntypes;
  for (int32_t k = 0; k < nt * nt; k++) {
    if (h->ty_rc[k] == 0.0 && h->lj_rcf[k] == 0.0) continue;  // (a pair of types the list leaves out)
    if (!(h->lj_rcf[k] <= h->ty_rc[k] - skin)) return fail(h, NL_ERR_ARG);
  }
  return NL_OK;
}

// What every entry point of a consumer does before its launch, and the launch (the Lennard-Jones, table, EAM and histogram
// calls; nl_pair_vectors has an order of its own, pair_vectors_call):
//   the arguments (NL_ERR_ARG, a null handle included); args_ok: the call's own;
//   synchronous: consumer_ready, then reach(0.0), the call's own preconditions and what it needs of the list;
//   enqueue (no wait: stream-ordered behind the update, or completed build, whose list it reads): reach(skin) first (what a
//   list reused within the skin guarantees), then consumer_ready; the kernels take the build's status word;
//   launch(stream, status).
template <typename REACH, typename LAUNCH>
int consumer_call(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* out_dev, bool args_ok, void* stream, bool enqueue,
                  REACH&& reach, LAUNCH&& launch) {
  if (!h || !q_dev || !out_dev || (q_stride != 3 && q_stride != 4) || !args_ok) return fail(h, NL_ERR_ARG);
  const hipStream_t s = (hipStream_t)stream;
  if (enqueue) {
    if (int rc = reach(h->skin)) return rc;
    if (int rc = consumer_ready(h, s, true)) return rc;
  } else {
    if (int rc = consumer_ready(h, s, false)) return rc;
    if (int rc = reach(0.0)) return rc;
  }
  HIPCHK(h, hipSetDevice(h->device));
  return launch(s, enqueue ? h->status : nullptr);
}

// The eight Lennard-Jones entry points (nl_lj_forces, nl_lj_virial, each _typed and _enqueue).  The reach: rc_force within
// the list's rc, or lj_typed_check.
template <typename OUT>
int lj_call(nl_handle_t h, const void* q_dev, int32_t q_stride, const double* lj, OUT* out_dev, void* stream, bool enqueue,
            int (*launch)(nl_handle_t, const void*, int32_t, const double*, OUT*, hipStream_t, const uint32_t*)) {
  return consumer_call(
      h, q_dev, q_stride, out_dev, !lj || (lj[2] > 0 && lj[1] > 0), stream, enqueue,
      [&](double skin) -> int {
        if (!lj) return lj_typed_check(h, skin);
        return lj[2] <= h->rc - skin ? NL_OK : fail(h, NL_ERR_ARG);  // the list does not reach that far (rc - 0.0 is rc, exactly)
      },
      [&](hipStream_t s, const uint32_t* status) { return launch(h, q_dev, q_stride, lj, out_dev, s, status); });
}
// ... and those of another pair function (nl_table_*, nl_eam_*), with its own reach.
template <typename OUT>
int pair_call(nl_handle_t h, const void* q_dev, int32_t q_stride, OUT* out_dev, void* stream, bool enqueue,
              int (*launch)(nl_handle_t, const void*, int32_t, OUT*, hipStream_t, const uint32_t*), int (*reach)(nl_handle_t, double)) {
  return consumer_call(h, q_dev, q_stride, out_dev, true, stream, enqueue, [&](double skin) { return reach(h, skin); },
                       [&](hipStream_t s, const uint32_t* status) { return launch(h, q_dev, q_stride, out_dev, s, status); });
}

}  // namespace

extern "C" {

int nl_lj_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force, void* f_dev,
                 void* stream) {
  const double lj[3] = {epsilon, sigma, rc_force};
  return lj_call(h, q_dev, q_stride, lj, f_dev, stream, false, lj_launch);
}
int nl_lj_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force,
                         void* f_dev, void* stream) {
  const double lj[3] = {epsilon, sigma, rc_force};
  return lj_call(h, q_dev, q_stride, lj, f_dev, stream, true, lj_launch);
}
int nl_lj_forces_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return lj_call(h, q_dev, q_stride, nullptr, f_dev, stream, false, lj_launch);
}
int nl_lj_forces_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  return lj_call(h, q_dev, q_stride, nullptr, f_dev, stream, true, lj_launch);
}

}  // extern "C"
