// nl_types.inc -- per-type cut-offs (nl_set_type_cutoffs): the cut-off of a pair taken from a symmetric table over the
// particle types of a mixture (Kob-Andersen, coarse-grained beads of several sizes, solvent around solutes), applied when
// the list is built, so that every consumer sees the list of the mixture.  And its consumer, typed Lennard-Jones forces.
//   The table   types[n] (input order, device copy, relabelled by the first nl_resort after a build) and rc2[a][b] in
//               the position type: the largest T <= rc_ab * rc_ab in double, as Grid::rc2 rounds the handle's rc.
//   The stage   the filter stage of nl_exclude.inc with a second predicate: the search writes the unfiltered list into
//               kp_pre / list_pre; k_type_count counts what each row keeps, the row scan makes key_pointer (META_KEPT),
//               k_type_compact copies the kept entries.  An entry (row i, partner j) is kept iff !(r2 > rc2[t_i][t_j])
//               and -- with an exclusion table as well (EXCL) -- {i, j} is not excluded: one pass, one predicate.
//               r2 is the value the search tested: both particles at the image the binning stored them at
//               (local_cell), the partner shifted by -+L across the periodic face the stencil reached it through
//               (segment_cells: a face of the i-cell's row of cells on an axis of the mask), (dx^2 + dy^2) + dz^2 in T.
//               A wave takes TYPE_ROWS consecutive rows at once: their entries are contiguous in list_pre, and lane r
//               holds row r's position, type and faces, which an entry fetches with ds_bpermute.
// Builds without a type table launch none of this.  Included at the end of nl_api.hip.

namespace {

constexpr int TYPE_THREADS = 256;
constexpr int TYPE_ROWS = 8;  // rows a wave takes at once (a row of the cfg-2 half list holds ~75 entries)

template <typename T> struct TypeArgs {
  Grid<T> g;                        // the build's binning (local_cell); g.gate = the update's gate
  const T* __restrict__ q;          // the caller's positions of the build
  int32_t stride, n, n_rows;
  const int32_t* __restrict__ types;  // [n], 0 <= t < ntypes (validated when set)
  const T* __restrict__ rc2;          // [NL_MAX_TYPES][NL_MAX_TYPES]
  int32_t ntypes;
  const int32_t* __restrict__ ex_off;  // EXCL: the exclusion table (nl_exclude.inc)
  const int32_t* __restrict__ ex_ids;
  int64_t capacity;
};

// A particle as the search saw it: its stored image (local_cell's shift on the axes of the mask, as the binning applies
// it) and its faces -- bit 2d: its cell is the first along axis d, bit 2d + 1: the last (axes of the mask only).
template <typename T, bool PBC>
__device__ __forceinline__ int32_t type_frame(const TypeArgs<T>& a, int32_t i, T& x, T& y, T& z) {
  load_xyz(a.q, a.stride, i, x, y, z);
  if constexpr (!PBC) return 0;
  int32_t lz = 0, row = 0;
  T sh[3];
  const int32_t c = local_cell(a.g, x, y, z, &lz, &row, sh);  // (a rejected particle fails its build: its faces do not matter)
  const int32_t ci[3] = {c - row * a.g.m[0], row - lz * a.g.m[1], lz};
  if (a.g.pbc & 1) x = add_rn(x, sh[0]);
  if (a.g.pbc & 2) y = add_rn(y, sh[1]);
  if (a.g.pbc & 4) z = add_rn(z, sh[2]);
  int32_t faces = 0;
#pragma unroll
  for (int d = 0; d < 3; d++)
    if ((a.g.pbc >> d) & 1) faces |= (ci[d] == 0 ? 1 : 0) << (2 * d) | (ci[d] == a.g.m[d] - 1 ? 2 : 0) << (2 * d);
  return faces;
}

// The face a partner with faces fj is reached through from a row with faces fi along axis d: -1 where the row's cell is
// the first and the partner's the last (the stencil reached it through the low face), +1 the other way round, else 0
// (m >= 3: never both).  The partner is shifted by S(w) = w_a a + w_b b + w_c c (lattice_shift): -+L_d in an orthogonal box.
__device__ __forceinline__ int32_t type_face_w(int32_t fi, int32_t fj, int d) {
  const int32_t lo_i = (fi >> (2 * d)) & 1, hi_i = (fi >> (2 * d + 1)) & 1;
  const int32_t lo_j = (fj >> (2 * d)) & 1, hi_j = (fj >> (2 * d + 1)) & 1;
  return (lo_i & hi_j) ? -1 : (hi_i & lo_j) ? 1 : 0;
}

template <typename T> __device__ __forceinline__ T shfl_t(T v, int src) {
  if constexpr (sizeof(T) == 4) {
    return __int_as_float(__shfl(__float_as_int(v), src, WAVE));
  } else {
    const int lo = __shfl(__double2loint(v), src, WAVE), hi = __shfl(__double2hiint(v), src, WAVE);
    return __hiloint2double(hi, lo);
  }
}

// Is v one of the ids of the sorted segment ids[xb, xb + ne)?
__device__ __forceinline__ bool type_excluded(const int32_t* __restrict__ ids, int32_t xb, int32_t ne, int32_t v) {
  int32_t lo = xb, hi = xb + ne;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (ids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < xb + ne && ids[lo] == v;
}

// The rows of a wave's chunk: lane r < nr holds row r0 + r.
template <typename T> struct TypeRows {
  int64_t beg[TYPE_ROWS];  // (uniform) first entry of every row of the chunk in list_pre
  int64_t b, e;            // (uniform) the chunk's entries [b, e), within the list's capacity
  int32_t nr;
  T x, y, z;               // lane r: row r's stored position ...
  int32_t tf;              // ... its type | faces << 8
  int32_t xb, ne;          // ... EXCL: its excluded ids
};

template <typename T, typename OFF, bool PBC, bool EXCL>
__device__ __forceinline__ void type_rows(const TypeArgs<T>& a, const OFF* __restrict__ kp_pre, int32_t r0, int lane, TypeRows<T>& r) {
  r.nr = min(TYPE_ROWS, a.n_rows - r0);
  const int32_t row = r0 + min(lane, r.nr - 1);
  const int64_t b = (int64_t)kp_pre[row];
  r.x = r.y = r.z = (T)0, r.tf = 0, r.xb = 0, r.ne = 0;
  if (lane < r.nr) {
    const int32_t faces = type_frame<T, PBC>(a, row, r.x, r.y, r.z);
    r.tf = (a.types[row] & (NL_MAX_TYPES - 1)) | faces << 8;
    if constexpr (EXCL) r.xb = a.ex_off[row], r.ne = a.ex_off[row + 1] - r.xb;
  }
#pragma unroll
  for (int k = 0; k < TYPE_ROWS; k++) {
    const int src = min(k, r.nr - 1);
    r.beg[k] = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int32_t)((uint64_t)b >> 32), src) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int32_t)b, src));
  }
  const int64_t e = (int64_t)kp_pre[r0 + r.nr];  // (uniform address)
  r.b = max(r.beg[0], (int64_t)0);
  r.e = min(e, a.capacity);  // (entries past the capacity were never written: such a build fails, and they are only not read)
}

// THE predicate of the stage, for entry k of the chunk (count and compact both call it).  Returns the partner in j.
template <typename T, bool PBC, bool EXCL>
__device__ __forceinline__ bool type_keep(const TypeArgs<T>& a, const TypeRows<T>& r, const int32_t* __restrict__ list_pre,
                                          const T* thr, int64_t k, int32_t& j, int32_t& lr) {
  const bool valid = k < r.e;
  lr = 0;
#pragma unroll
  for (int t = 1; t < TYPE_ROWS; t++) lr += (t < r.nr && k >= r.beg[t]) ? 1 : 0;
  j = valid ? list_pre[k] : 0;
  const bool in = valid && (uint32_t)j < (uint32_t)a.n;  // (an entry of a failed build may be anything)
  if (!in) j = 0;
  T xj, yj, zj;
  const int32_t fj = type_frame<T, PBC>(a, j, xj, yj, zj);
  const int32_t tj = a.types[j] & (NL_MAX_TYPES - 1);
  const T xi = shfl_t(r.x, lr), yi = shfl_t(r.y, lr), zi = shfl_t(r.z, lr);
  const int32_t tf = __shfl(r.tf, lr, WAVE);
  if constexpr (PBC) {
    const int32_t fi = tf >> 8;
    T sw[3];  // the lattice vector of the faces, as the search staged the partner
    lattice_shift(a.g.lat, (type_face_w(fi, fj, 0) + 1) | (type_face_w(fi, fj, 1) + 1) << 2 | (type_face_w(fi, fj, 2) + 1) << 4, sw);
    if (a.g.pbc & 1) xj = add_rn(xj, sw[0]);
    if (a.g.pbc & 2) yj = add_rn(yj, sw[1]);
    if (a.g.pbc & 4) zj = add_rn(zj, sw[2]);
  }
  const T dx = sub_rn(xj, xi), dy = sub_rn(yj, yi), dz = sub_rn(zj, zi);
  const T r2 = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
  bool keep = in && !(r2 > thr[(tf & (NL_MAX_TYPES - 1)) * NL_MAX_TYPES + tj]);
  if constexpr (EXCL) {
    const int32_t xb = __shfl(r.xb, lr, WAVE), ne = __shfl(r.ne, lr, WAVE);
    if (keep && ne > 0) keep = !type_excluded(a.ex_ids, xb, ne, j);
  }
  return keep;
}

// The thresholds of the table's rows into LDS (rows past ntypes are never read: types are validated)
template <typename T> __device__ __forceinline__ void type_load_thr(const TypeArgs<T>& a, T* thr) {
  for (int32_t k = threadIdx.x; k < a.ntypes * NL_MAX_TYPES; k += TYPE_THREADS) thr[k] = a.rc2[k];
  __syncthreads();
}

// count[row] = entries of the unfiltered row that the stage keeps
template <typename T, typename OFF, bool PBC, bool EXCL>
__global__ void __launch_bounds__(TYPE_THREADS) k_type_count(TypeArgs<T> a, const OFF* __restrict__ kp_pre, const int32_t* __restrict__ list_pre,
                                                            int32_t* __restrict__ count) {
  if (gate_closed(a.g.gate)) return;  // (nl_update_list: no build this time)
  __shared__ T thr[NL_MAX_TYPES * NL_MAX_TYPES];
  type_load_thr(a, thr);
  const int lane = threadIdx.x & 63;
  const int32_t chunks = (a.n_rows + TYPE_ROWS - 1) / TYPE_ROWS, waves = gridDim.x * (TYPE_THREADS / WAVE);
  for (int32_t c = blockIdx.x * (TYPE_THREADS / WAVE) + (threadIdx.x >> 6); c < chunks; c += waves) {
    const int32_t r0 = c * TYPE_ROWS;
    TypeRows<T> r;
    type_rows<T, OFF, PBC, EXCL>(a, kp_pre, r0, lane, r);
    int32_t kept = 0;  // lane t: row t's
    for (int64_t k = r.b + lane; k - lane < r.e; k += WAVE) {
      int32_t j, lr;
      const bool keep = type_keep<T, PBC, EXCL>(a, r, list_pre, thr, k, j, lr);
#pragma unroll
      for (int t = 0; t < TYPE_ROWS; t++) {
        const int32_t m = __builtin_popcountll(__ballot(keep && lr == t));
        kept += lane == t ? m : 0;
      }
    }
    if (lane < r.nr) count[r0 + lane] = kept;
  }
}

// list[key_pointer[r0] ...] = the kept entries of the chunk's rows, in their order (ballot + mbcnt): the rows are
// consecutive, so are their kept entries
template <typename T, typename OFF, bool PBC, bool EXCL>
__global__ void __launch_bounds__(TYPE_THREADS) k_type_compact(TypeArgs<T> a, const OFF* __restrict__ kp_pre, const int32_t* __restrict__ list_pre,
                                                              const OFF* __restrict__ kp, int32_t* __restrict__ list) {
  if (gate_closed(a.g.gate)) return;  // (nl_update_list: no build this time)
  __shared__ T thr[NL_MAX_TYPES * NL_MAX_TYPES];
  type_load_thr(a, thr);
  const int lane = threadIdx.x & 63;
  const int32_t chunks = (a.n_rows + TYPE_ROWS - 1) / TYPE_ROWS, waves = gridDim.x * (TYPE_THREADS / WAVE);
  for (int32_t c = blockIdx.x * (TYPE_THREADS / WAVE) + (threadIdx.x >> 6); c < chunks; c += waves) {
    const int32_t r0 = c * TYPE_ROWS;
    TypeRows<T> r;
    type_rows<T, OFF, PBC, EXCL>(a, kp_pre, r0, lane, r);
    int64_t dst = (int64_t)kp[r0];
    for (int64_t k = r.b + lane; k - lane < r.e; k += WAVE) {
      int32_t j, lr;
      const bool keep = type_keep<T, PBC, EXCL>(a, r, list_pre, thr, k, j, lr);
      const uint64_t mask = __ballot(keep);
      const int64_t d = dst + lanes_below(mask);
      if (keep && d >= 0 && d < a.capacity) list[d] = j;
      dst += __builtin_popcountll(mask);
    }
  }
}

// 0 <= types[i] < ntypes for every i < n, else *bad = 1
__global__ void __launch_bounds__(256) k_type_check(const int32_t* __restrict__ types, int32_t n, int32_t ntypes, uint32_t* __restrict__ bad) {
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (types[i] < 0 || types[i] >= ntypes) atomicOr(bad, 1u);
}

template <typename T, typename OFF, bool PBC, bool EXCL> int launch_types_v(nl_handle_t h, int32_t n_rows, hipStream_t s) {
  TypeArgs<T> a;
  a.g = make_grid<T>(h, h->args, h->plan.pbc);
  a.q = static_cast<const T*>(h->args.q);
  a.stride = h->args.stride, a.n = h->args.n, a.n_rows = n_rows;
  a.types = h->ty_types, a.rc2 = static_cast<const T*>(h->ty_rc2), a.ntypes = h->ty_ntypes;
  a.ex_off = h->ex_off, a.ex_ids = h->ex_ids;
  a.capacity = h->capacity;
  const OFF* kp_pre = static_cast<const OFF*>(h->kp_pre);
  const int32_t chunks = (n_rows + TYPE_ROWS - 1) / TYPE_ROWS;
  const int32_t grid = std::max(1, std::min((chunks + 3) / 4, 16 * h->num_cus));
  if (n_rows > 0) hipLaunchKernelGGL((k_type_count<T, OFF, PBC, EXCL>), dim3(grid), dim3(TYPE_THREADS), 0, s, a, kp_pre, h->list_pre, h->count);
  if (int rc = launch_scan(h, h->count, n_rows, static_cast<OFF*>(h->key_pointer), h->totals + 2, s, h->status + META_KEPT)) return rc;
  if (n_rows > 0)
    hipLaunchKernelGGL((k_type_compact<T, OFF, PBC, EXCL>), dim3(grid), dim3(TYPE_THREADS), 0, s, a, kp_pre, h->list_pre,
                       static_cast<const OFF*>(h->key_pointer), h->list);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

template <typename T, typename OFF> int launch_types_w(nl_handle_t h, int32_t n_rows, hipStream_t s) {
  const bool pbc = h->plan.pbc != 0, excl = h->ex_ids != nullptr;
  if (pbc) return excl ? launch_types_v<T, OFF, true, true>(h, n_rows, s) : launch_types_v<T, OFF, true, false>(h, n_rows, s);
  return excl ? launch_types_v<T, OFF, false, true>(h, n_rows, s) : launch_types_v<T, OFF, false, false>(h, n_rows, s);
}

template <typename T> int launch_types_t(nl_handle_t h, int32_t n_rows, hipStream_t s) {
  return h->plan.wide ? launch_types_w<T, int64_t>(h, n_rows, s) : launch_types_w<T, int32_t>(h, n_rows, s);
}

// (declared at the top of nl_api.hip) The filter stage of the handle's build: the typed stage (with the exclusions in
// it) where a type table is set, else the exclusion stage.
int launch_filter(nl_handle_t h, int32_t n_rows, hipStream_t s) {
  if (!h->ty_types) return launch_exclude(h, n_rows, s);
  return h->dtype == NL_F32 ? launch_types_t<float>(h, n_rows, s) : launch_types_t<double>(h, n_rows, s);
}

void types_clear(nl_handle_t h) {
  for (void* b : {(void*)h->ty_types, h->ty_rc2})
    if (b) (void)hipFree(b);
  h->ty_types = nullptr, h->ty_rc2 = nullptr;
  h->ty_n = 0, h->ty_ntypes = 0, h->ty_cap = 0;
  h->ty_gen++;
  h->buffers_epoch++;
  if (!h->ex_ids) filter_release(h);
}

// (declared at the top of nl_api.hip) The types in the cell order of the last build: types[s] <- types[order[s]], in
// the same buffer (a graph the caller captured keeps reading it).
int types_relabel(nl_handle_t h) {
  const int32_t n = h->ty_n;
  int32_t* tmp = nullptr;
  hipStream_t s = h->own_stream;
  HIPCHK(h, hipDeviceSynchronize());  // (replays of a graph the caller captured may still read the types)
  if (hipMalloc(reinterpret_cast<void**>(&tmp), 4 * ((size_t)n + 16)) != hipSuccess) return fail(h, NL_ERR_NOMEM);
  int rc = NL_OK;
  if (n > 0) {
    hipLaunchKernelGGL(k_gather_words<1>, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(h->ty_types),
                       h->sorted_row, n, reinterpret_cast<uint32_t*>(tmp));
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h->ty_types, tmp, 4 * (size_t)n, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = fail(h, NL_ERR_HIP);
  }
  (void)hipFree(tmp);
  h->ty_gen++;
  return rc;
}

// ------------------------------------------------------------------------------------------ typed Lennard-Jones
// k_lj with the parameters of the pair's types: lane t < ntypes holds eps4, sig2 and rcf2 of (t_row, t), an entry picks
// them by its partner's type with ds_bpermute.  Everything else as k_lj (images, NaN on a failed build, half / full).
template <typename T, bool HALF, typename OFF, bool TRI>
__global__ void __launch_bounds__(256) k_lj_typed(const T* __restrict__ q, int32_t stride, const OFF* __restrict__ kp,
                                                  const int32_t* __restrict__ list, int32_t n, const int32_t* __restrict__ types,
                                                  const T* __restrict__ par, T* __restrict__ f, T Lx, T Ly, T Lz,
                                                  const uint32_t* __restrict__ status, T xy, T xz, T yz) {
  const int32_t row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= n) return;
  if (status && *status != 0u) {  // (uniform: every row of the launch takes this branch)
    if (lane == 0) {
      const T nan = (T)NAN;
      f[(size_t)row * 4 + 0] = nan, f[(size_t)row * 4 + 1] = nan, f[(size_t)row * 4 + 2] = nan, f[(size_t)row * 4 + 3] = nan;
    }
    return;
  }
  constexpr int NT2 = NL_MAX_TYPES * NL_MAX_TYPES;
  const int32_t ti = types[row] & (NL_MAX_TYPES - 1);
  const int32_t at = ti * NL_MAX_TYPES + (lane & (NL_MAX_TYPES - 1));
  const T my_eps4 = par[at], my_sig2 = par[NT2 + at], my_rcf2 = par[2 * NT2 + at];
  T xi, yi, zi;
  load_xyz(q, stride, row, xi, yi, zi);
  T ax = 0, ay = 0, az = 0, ae = 0;
  const OFF b = kp[row], e = kp[row + 1];
  for (OFF k = b + lane; k - lane < e; k += 64) {
    const bool valid = k < e;
    const int32_t j = valid ? list[k] : row;
    const int32_t tj = types[j] & (NL_MAX_TYPES - 1);
    const T eps4 = shfl_t(my_eps4, tj), sig2 = shfl_t(my_sig2, tj), rcf2 = shfl_t(my_rcf2, tj);  // (every lane: bpermute)
    if (!valid) continue;
    T xj, yj, zj;
    load_xyz(q, stride, j, xj, yj, zj);
    T fx, fy, fz, pe;
    bool in;
    T dx = xi - xj, dy = yi - yj, dz = zi - zj;
    lj_image<T, TRI>(dx, dy, dz, Lx, Ly, Lz, xy, xz, yz);
    lj_pair<T>(dx, dy, dz, eps4, sig2, rcf2, fx, fy, fz, pe, in);
    ax += fx, ay += fy, az += fz, ae += (T)0.5 * pe;
    if (HALF && in) {
      atomicAdd(&f[(size_t)j * 4 + 0], -fx);
      atomicAdd(&f[(size_t)j * 4 + 1], -fy);
      atomicAdd(&f[(size_t)j * 4 + 2], -fz);
      atomicAdd(&f[(size_t)j * 4 + 3], (T)0.5 * pe);
    }
  }
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

template <typename T, typename OFF>
int lj_typed_launch(nl_handle_t h, const void* q_dev, int32_t stride, void* f_dev, hipStream_t s, const uint32_t* status = nullptr) {
  const int32_t n = h->n;
  if (n == 0) return NL_OK;
  const int32_t nbw = (int32_t)(((int64_t)n * 64 + 255) / 256);
  const Box& b = h->plan.box;  // (the build's box, as k_lj)
  const T Lx = (h->plan.pbc & 1) ? (T)b.L[0] : (T)0, Ly = (h->plan.pbc & 2) ? (T)b.L[1] : (T)0, Lz = (h->plan.pbc & 4) ? (T)b.L[2] : (T)0;
  const T xy = (T)b.xy, xz = (T)b.xz, yz = (T)b.yz;
  const T* par = static_cast<const T*>(h->lj_par);
  auto launch = [&](auto half, auto tri) {
    hipLaunchKernelGGL((k_lj_typed<T, decltype(half)::value, OFF, decltype(tri)::value>), dim3(nbw), dim3(256), 0, s,
                       static_cast<const T*>(q_dev), stride, static_cast<const OFF*>(h->key_pointer), h->list, n, h->ty_types, par,
                       static_cast<T*>(f_dev), Lx, Ly, Lz, status, xy, xz, yz);
  };
  if (!h->plan.full) HIPCHK(h, hipMemsetAsync(f_dev, 0, sizeof(T) * 4 * (size_t)n, s));
  if (h->plan.tilt) h->plan.full ? launch(std::false_type(), std::true_type()) : launch(std::true_type(), std::true_type());
  else h->plan.full ? launch(std::false_type(), std::false_type()) : launch(std::true_type(), std::false_type());
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

int lj_typed_dispatch(nl_handle_t h, const void* q_dev, int32_t stride, void* f_dev, hipStream_t s, const uint32_t* status) {
  if (h->plan.wide)
    return h->dtype == NL_F32 ? lj_typed_launch<float, int64_t>(h, q_dev, stride, f_dev, s, status)
                              : lj_typed_launch<double, int64_t>(h, q_dev, stride, f_dev, s, status);
  return h->dtype == NL_F32 ? lj_typed_launch<float, int32_t>(h, q_dev, stride, f_dev, s, status)
                            : lj_typed_launch<double, int32_t>(h, q_dev, stride, f_dev, s, status);
}

// The typed forces' preconditions beyond the untyped ones: a type table and parameters of its ntypes, and rc_force_ab
// within rc_ab (less the skin for the enqueue variant, whose list may be reused).
int lj_typed_check(nl_handle_t h, double skin) {
  if (!h->ty_types || !h->lj_par) return fail(h, NL_ERR_STATE);
  if (h->lj_ntypes != h->ty_ntypes) return fail(h, NL_ERR_ARG);
  const int32_t nt = h->ty_ntypes;
  for (int32_t k = 0; k < nt * nt; k++)
    if (!(h->lj_rcf[k] <= h->ty_rc[k] - skin)) return fail(h, NL_ERR_ARG);
  return NL_OK;
}

}  // namespace

extern "C" {

int nl_set_type_cutoffs(nl_handle_t h, const int32_t* types_dev, int32_t n, int32_t ntypes, const double* rc_host) {
  if (!h) return NL_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  if (!types_dev || ntypes == 0) {
    if (h->ty_types) types_clear(h);
    h->upd_valid = false;
    return NL_OK;
  }
  if (ntypes < 1 || ntypes > NL_MAX_TYPES || n < 0 || n > h->n_max || !rc_host) return fail(h, NL_ERR_ARG);
  for (int32_t a = 0; a < ntypes; a++)
    for (int32_t b = 0; b < ntypes; b++) {
      const double v = rc_host[a * ntypes + b];
      if (!(v >= 0.0 && v <= h->rc) || v != rc_host[b * ntypes + a]) return fail(h, NL_ERR_ARG);
    }
  HIPCHK(h, hipDeviceSynchronize());  // (the caller's types may come from any stream)
  hipStream_t s = h->own_stream;
  {
    uint32_t* bad = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&bad), 16) != hipSuccess) return fail(h, NL_ERR_NOMEM);
    uint32_t b = 0;
    hipError_t e = hipMemsetAsync(bad, 0, 16, s);
    if (e == hipSuccess && n > 0) {
      hipLaunchKernelGGL(k_type_check, dim3((uint32_t)std::max(1, std::min((n + 255) / 256, 8 * h->num_cus))), dim3(256), 0, s, types_dev, n, ntypes, bad);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(bad);
    HIPCHK(h, e);
    if (b) return fail(h, NL_ERR_ARG);
  }
  // the table, in its buffers where they hold it (a graph the caller captured keeps reading them)
  const bool f32 = h->dtype == NL_F32;
  const size_t thr_bytes = (f32 ? 4 : 8) * (size_t)NL_MAX_TYPES * NL_MAX_TYPES;
  if (!h->ty_types || h->ty_cap < (int64_t)n) {
    void* old = h->ty_types;
    int32_t* p = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&p), 4 * ((size_t)h->n_max + 16)) != hipSuccess) return fail(h, NL_ERR_NOMEM);
    if (old) (void)hipFree(old);
    h->ty_types = p, h->ty_cap = h->n_max;
    h->buffers_epoch++;
  }
  if (!h->ty_rc2) {
    if (hipMalloc(&h->ty_rc2, thr_bytes) != hipSuccess) {
      types_clear(h);
      return fail(h, NL_ERR_NOMEM);
    }
    h->buffers_epoch++;
  }
  double thr_d[NL_MAX_TYPES * NL_MAX_TYPES] = {};
  float thr_f[NL_MAX_TYPES * NL_MAX_TYPES] = {};
  for (int32_t a = 0; a < ntypes; a++)
    for (int32_t b = 0; b < ntypes; b++) {
      const double r = rc_host[a * ntypes + b];
      thr_d[a * NL_MAX_TYPES + b] = r * r;  // (as Grid::rc2: the largest T <= rc_ab * rc_ab in double)
      thr_f[a * NL_MAX_TYPES + b] = floor_to_float(r * r);
    }
  if (n > 0) HIPCHK(h, hipMemcpyAsync(h->ty_types, types_dev, 4 * (size_t)n, hipMemcpyDeviceToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->ty_rc2, f32 ? (const void*)thr_f : (const void*)thr_d, thr_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipStreamSynchronize(s));
  for (int32_t k = 0; k < NL_MAX_TYPES * NL_MAX_TYPES; k++) h->ty_rc[k] = 0;
  for (int32_t a = 0; a < ntypes; a++)
    for (int32_t b = 0; b < ntypes; b++) h->ty_rc[a * ntypes + b] = rc_host[a * ntypes + b];
  h->ty_n = n, h->ty_ntypes = ntypes;
  h->ty_gen++;
  h->upd_valid = false;
  if (int rc = excl_reserve(h)) {  // no room for the unfiltered buffers: no table
    types_clear(h);
    return rc;
  }
  return NL_OK;
}

int nl_get_types(nl_handle_t h, const int32_t** types_dev, int32_t* n, int32_t* ntypes) {
  if (!h) return NL_ERR_ARG;
  if (!h->ty_types) return fail(h, NL_ERR_STATE);
  if (types_dev) *types_dev = h->ty_types;
  if (n) *n = h->ty_n;
  if (ntypes) *ntypes = h->ty_ntypes;
  return NL_OK;
}

int nl_set_lj_type_params(nl_handle_t h, int32_t ntypes, const double* epsilon, const double* sigma, const double* rc_force) {
  if (!h) return NL_ERR_ARG;
  if (!epsilon || !sigma || !rc_force) return fail(h, NL_ERR_ARG);
  if (!h->ty_types) return fail(h, NL_ERR_STATE);
  if (ntypes != h->ty_ntypes) return fail(h, NL_ERR_ARG);
  for (int32_t a = 0; a < ntypes; a++)
    for (int32_t b = 0; b < ntypes; b++) {
      const int32_t k = a * ntypes + b, t = b * ntypes + a;
      if (!std::isfinite(epsilon[k]) || !(sigma[k] > 0) || !std::isfinite(sigma[k]) || !(rc_force[k] > 0) ||
          !(rc_force[k] <= h->ty_rc[k]) || epsilon[k] != epsilon[t] || sigma[k] != sigma[t] || rc_force[k] != rc_force[t])
        return fail(h, NL_ERR_ARG);
    }
  HIPCHK(h, hipSetDevice(h->device));
  constexpr int NT2 = NL_MAX_TYPES * NL_MAX_TYPES;
  const bool f32 = h->dtype == NL_F32;
  const size_t bytes = (f32 ? 4 : 8) * 3 * (size_t)NT2;
  if (!h->lj_par) {
    HIPCHK(h, hipDeviceSynchronize());
    if (hipMalloc(&h->lj_par, bytes) != hipSuccess) return fail(h, NL_ERR_NOMEM);
  }
  double pd[3 * NT2] = {};
  float pf[3 * NT2] = {};
  for (int32_t a = 0; a < ntypes; a++)
    for (int32_t b = 0; b < ntypes; b++) {
      const int32_t k = a * ntypes + b, at = a * NL_MAX_TYPES + b;
      // (as lj_launch rounds its scalars)
      pd[at] = 4.0 * epsilon[k], pd[NT2 + at] = sigma[k] * sigma[k], pd[2 * NT2 + at] = rc_force[k] * rc_force[k];
      pf[at] = (float)pd[at], pf[NT2 + at] = (float)pd[NT2 + at], pf[2 * NT2 + at] = (float)pd[2 * NT2 + at];
    }
  // synchronous (the device may still replay a graph that reads the old parameters): the enqueue variant copies nothing
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(h->lj_par, f32 ? (const void*)pf : (const void*)pd, bytes, hipMemcpyHostToDevice));
  for (int32_t k = 0; k < ntypes * ntypes; k++) h->lj_rcf[k] = rc_force[k];
  h->lj_ntypes = ntypes;
  return NL_OK;
}

int nl_lj_forces_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  if (!h || !q_dev || !f_dev || (q_stride != 3 && q_stride != 4)) return fail(h, NL_ERR_ARG);
  int rc = nl_synchronize(h);  // the list must be complete (and its build must have succeeded)
  if (rc) return rc;
  if (h->args.slab || h->n_rows != h->n) return fail(h, NL_ERR_STATE);  // ids must index q
  if ((rc = lj_typed_check(h, 0.0))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return lj_typed_dispatch(h, q_dev, q_stride, f_dev, (hipStream_t)stream, nullptr);
}

// nl_lj_forces_typed without the wait: stream-ordered behind the update (or completed build) whose list it reads.
int nl_lj_forces_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream) {
  if (!h || !q_dev || !f_dev || (q_stride != 3 && q_stride != 4)) return fail(h, NL_ERR_ARG);
  if (int rc = lj_typed_check(h, h->skin)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!h->pending && !h->built) return fail(h, NL_ERR_STATE);  // no build, or one the host has seen fail
  if (h->pending && (!h->last_update || s != h->last_stream)) return fail(h, NL_ERR_STATE);
  if (h->args.slab || h->n_rows != h->n) return fail(h, NL_ERR_STATE);  // ids must index q
  HIPCHK(h, hipSetDevice(h->device));
  return lj_typed_dispatch(h, q_dev, q_stride, f_dev, s, h->status);
}

}  // extern "C"
