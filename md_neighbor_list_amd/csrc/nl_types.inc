// nl_types.inc -- per-type cut-offs (nl_set_type_cutoffs): the cut-off of a pair taken from a symmetric table over the
// particle types of a mixture (Kob-Andersen, coarse-grained beads of several sizes, solvent around solutes), applied when
// the list is built, so that every consumer sees the list of the mixture (typed Lennard-Jones forces: nl_consumer.inc).
//   The table   types[n] (input order, device copy, relabelled by the first nl_resort after a build) and rc2[a][b] in
//               the position type: the largest T <= rc_ab * rc_ab in double, as Grid::rc2 rounds the handle's rc.
//   The stage   the filter stage of nl_exclude.inc with a second predicate: the search writes the unfiltered list into
//               kp_pre / list_pre; k_type_count counts what each row keeps, the row scan makes key_pointer (META_KEPT),
//               k_type_compact copies the kept entries.  An entry (row i, partner j) is kept iff !(r2 > rc2[t_i][t_j])
//               and -- with an exclusion table as well (EXCL) -- {i, j} is not excluded: one pass, one predicate.
//               r2 is the value the search tested: both particles at the image the binning stored them at
//               (particle_frame), the partner shifted by -+L across the periodic face the stencil reached it through
//               (face_w), (dx^2 + dy^2) + dz^2 in T.
//               A wave takes a chunk of STAGE_ROWS consecutive rows at once (row_chunk, nl_stage.hpp), and lane r
//               holds row r's position, type and frame, which an entry fetches with ds_bpermute.
// Builds without a type table launch none of this.  Included at the end of nl_api.hip.

namespace {

template <typename T, typename OFF> struct TypeArgs {
  Grid<T> g;                        // the build's binning (local_cell); g.gate = the update's gate
  const T* __restrict__ q;          // the caller's positions of the build
  int32_t stride, n, n_rows;
  const OFF* __restrict__ kp_pre;   // the unfiltered offsets and list
  const int32_t* __restrict__ list_pre;
  const int32_t* __restrict__ types;  // [n], 0 <= t < ntypes (validated when set)
  const T* __restrict__ rc2;          // [NL_MAX_TYPES][NL_MAX_TYPES]
  int32_t ntypes;
  const int32_t* __restrict__ ex_off;  // EXCL: the exclusion table (nl_exclude.inc)
  const int32_t* __restrict__ ex_ids;
  int64_t capacity;
};

// A particle as the search saw it: its stored image (local_cell's shift on the axes of the mask, as the binning applies
// it) and its frame (particle_frame).
template <bool PBC, typename T>
__device__ __forceinline__ uint32_t type_frame(const Grid<T>& g, const T* __restrict__ q, int32_t stride, int32_t i, T& x, T& y, T& z) {
  load_xyz(q, stride, i, x, y, z);
  if constexpr (!PBC) return 0u;
  T sh[3] = {0, 0, 0};
  const uint32_t frame = particle_frame(g, x, y, z, sh);
  if (g.pbc & 1) x = add_rn(x, sh[0]);
  if (g.pbc & 2) y = add_rn(y, sh[1]);
  if (g.pbc & 4) z = add_rn(z, sh[2]);
  return frame;
}

// The rows of a wave's chunk: lane r < c.nr holds row r0 + r.
template <typename T> struct TypeRows {
  RowChunk c;
  T x, y, z;       // lane r: row r's stored position ...
  int32_t tf;      // ... its type | frame << 8
  int32_t xb, ne;  // ... EXCL: its excluded ids
};

template <bool PBC, bool EXCL, typename T, typename OFF>
__device__ __forceinline__ void type_rows(const TypeArgs<T, OFF>& a, int32_t r0, int lane, TypeRows<T>& r) {
  row_chunk<OFF>(a.kp_pre, a.n_rows, a.capacity, r0, lane, r.c);
  r.x = r.y = r.z = (T)0, r.tf = 0, r.xb = 0, r.ne = 0;
  if (lane < r.c.nr) {
    const int32_t row = r0 + lane;
    const uint32_t frame = type_frame<PBC>(a.g, a.q, a.stride, row, r.x, r.y, r.z);
    r.tf = (a.types[row] & (NL_MAX_TYPES - 1)) | (int32_t)(frame << 8);
    if constexpr (EXCL) r.xb = a.ex_off[row], r.ne = a.ex_off[row + 1] - r.xb;
  }
}

// THE predicate of the stage, for entry k of the chunk (both passes call it).  Returns the partner in j, the local row in lr.
template <bool PBC, bool EXCL, typename T, typename OFF>
__device__ __forceinline__ bool type_keep(const TypeArgs<T, OFF>& a, const TypeRows<T>& r, const T* thr, int64_t k, int32_t& j, int32_t& lr) {
  const bool valid = k < r.c.e;
  lr = chunk_row<OFF>(r.c, k);
  j = valid ? a.list_pre[k] : 0;
  const bool in = valid && (uint32_t)j < (uint32_t)a.n;  // (an entry of a failed build may be anything)
  if (!in) j = 0;
  T xj, yj, zj;
  const uint32_t fj = type_frame<PBC>(a.g, a.q, a.stride, j, xj, yj, zj);
  const int32_t tj = a.types[j] & (NL_MAX_TYPES - 1);
  const T xi = shfl_t(r.x, lr), yi = shfl_t(r.y, lr), zi = shfl_t(r.z, lr);
  const int32_t tf = __shfl(r.tf, lr, WAVE);
  if constexpr (PBC) {
    const uint32_t fi = (uint32_t)tf >> 8;
    T sw[3];  // the lattice vector of the faces, as the search staged the partner
    lattice_shift(a.g.lat, (face_w(fi, fj, 0) + 1) | (face_w(fi, fj, 1) + 1) << 2 | (face_w(fi, fj, 2) + 1) << 4, sw);
    if (a.g.pbc & 1) xj = add_rn(xj, sw[0]);
    if (a.g.pbc & 2) yj = add_rn(yj, sw[1]);
    if (a.g.pbc & 4) zj = add_rn(zj, sw[2]);
  }
  const T dx = sub_rn(xj, xi), dy = sub_rn(yj, yi), dz = sub_rn(zj, zi);
  const T r2 = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
  bool keep = in && !(r2 > thr[(tf & (NL_MAX_TYPES - 1)) * NL_MAX_TYPES + tj]);
  if constexpr (EXCL) {
    const int32_t xb = __shfl(r.xb, lr, WAVE), ne = __shfl(r.ne, lr, WAVE);
    if (keep && ne > 0) keep = !sorted_contains(a.ex_ids, xb, ne, j);
  }
  return keep;
}

// Both passes of the stage, a chunk of rows per wave.  Count: count[row] = entries of the unfiltered row that the stage
// keeps.  COMPACT: list[kp[r0] ...] = the kept entries of the chunk's rows, in their order (ballot + mbcnt): the rows are
// consecutive, so are their kept entries.
template <bool PBC, bool EXCL, bool COMPACT, typename T, typename OFF>
__device__ __forceinline__ void type_pass(const TypeArgs<T, OFF>& a, int32_t* __restrict__ count, const OFF* __restrict__ kp,
                                          int32_t* __restrict__ list) {
  if (gate_closed(a.g.gate)) return;  // (nl_update_list: no build this time)
  __shared__ T thr[NL_MAX_TYPES * NL_MAX_TYPES];  // the table's rows (those past ntypes are never read: types are validated)
  for (int32_t k = threadIdx.x; k < a.ntypes * NL_MAX_TYPES; k += STAGE_THREADS) thr[k] = a.rc2[k];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int32_t chunks = (a.n_rows + STAGE_ROWS - 1) / STAGE_ROWS, waves = gridDim.x * (STAGE_THREADS / WAVE);
  for (int32_t c = blockIdx.x * (STAGE_THREADS / WAVE) + (threadIdx.x >> 6); c < chunks; c += waves) {
    const int32_t r0 = c * STAGE_ROWS;
    TypeRows<T> r;
    type_rows<PBC, EXCL>(a, r0, lane, r);
    int32_t kept = 0;  // (count) lane t: row t's
    int64_t dst = 0;   // (COMPACT)
    if constexpr (COMPACT) dst = (int64_t)kp[r0];
    for (int64_t k = r.c.b + lane; k - lane < r.c.e; k += WAVE) {
      int32_t j, lr;
      const bool keep = type_keep<PBC, EXCL>(a, r, thr, k, j, lr);
      if constexpr (COMPACT) {
        const uint64_t mask = __ballot(keep);
        const int64_t d = dst + lanes_below(mask);
        if (keep && d >= 0 && d < a.capacity) list[d] = j;
        dst += __builtin_popcountll(mask);
      } else {
#pragma unroll
        for (int t = 0; t < STAGE_ROWS; t++) {
          const int32_t m = __builtin_popcountll(__ballot(keep && lr == t));
          kept += lane == t ? m : 0;
        }
      }
    }
    if (!COMPACT && lane < r.c.nr) count[r0 + lane] = kept;
  }
}

template <typename T, typename OFF, bool PBC, bool EXCL>
__global__ void __launch_bounds__(STAGE_THREADS) k_type_count(TypeArgs<T, OFF> a, int32_t* __restrict__ count) {
  type_pass<PBC, EXCL, false>(a, count, static_cast<const OFF*>(nullptr), nullptr);
}
template <typename T, typename OFF, bool PBC, bool EXCL>
__global__ void __launch_bounds__(STAGE_THREADS) k_type_compact(TypeArgs<T, OFF> a, const OFF* __restrict__ kp, int32_t* __restrict__ list) {
  type_pass<PBC, EXCL, true>(a, nullptr, kp, list);
}

// 0 <= types[i] < ntypes for every i < n, else *bad = 1
__global__ void __launch_bounds__(256) k_type_check(const int32_t* __restrict__ types, int32_t n, int32_t ntypes, uint32_t* __restrict__ bad) {
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (types[i] < 0 || types[i] >= ntypes) atomicOr(bad, 1u);
}

// (declared at the top of nl_api.hip) The filter stage of the handle's build: the typed stage (with the exclusions in
// it) where a type table is set, else the exclusion stage.
int launch_filter(nl_handle_t h, int32_t n_rows, hipStream_t s) {
  if (!h->ty_types) return launch_exclude(h, n_rows, s);
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    TypeArgs<T, OFF> a;
    a.g = make_grid<T>(h, h->args, h->plan.pbc);
    a.q = static_cast<const T*>(h->args.q);
    a.stride = h->args.stride, a.n = h->args.n, a.n_rows = n_rows;
    a.kp_pre = static_cast<const OFF*>(h->kp_pre), a.list_pre = h->list_pre;
    a.types = h->ty_types, a.rc2 = static_cast<const T*>(h->ty_rc2), a.ntypes = h->ty_ntypes;
    a.ex_off = h->ex_off, a.ex_ids = h->ex_ids;
    a.capacity = h->capacity;
    const int32_t chunks = (n_rows + STAGE_ROWS - 1) / STAGE_ROWS;
    auto launch = [&](auto pbc, auto excl) {
      constexpr bool P = decltype(pbc)::value, E = decltype(excl)::value;
      return launch_passes<OFF>(h, n_rows, chunks, s, a, k_type_count<T, OFF, P, E>, k_type_compact<T, OFF, P, E>);
    };
    const bool excl = h->ex_ids != nullptr;
    if (h->plan.pbc != 0) return excl ? launch(std::true_type(), std::true_type()) : launch(std::true_type(), std::false_type());
    return excl ? launch(std::false_type(), std::true_type()) : launch(std::false_type(), std::false_type());
  });
}

void types_clear(nl_handle_t h) {
  h->ty_types.release(), h->ty_rc2.release();
  h->ty_n = 0, h->ty_ntypes = 0;
  h->ty_gen++;
  h->buffers_epoch++;
  if (!h->ex_ids) filter_release(h);
}

// (declared at the top of nl_api.hip) The types in the cell order of the last build: types[s] <- types[order[s]], in
// the same buffer (a graph the caller captured keeps reading it).
int types_relabel(nl_handle_t h) {
  const int32_t n = h->ty_n;
  DevBuf<int32_t> tmp;
  hipStream_t s = h->own_stream;
  HIPCHK(h, hipDeviceSynchronize());  // (replays of a graph the caller captured may still read the types)
  if (int rc = side_alloc(h, tmp, 4 * ((size_t)n + 16))) return rc;
  int rc = NL_OK;
  if (n > 0) {
    hipLaunchKernelGGL(k_gather_words<1>, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(h->ty_types.get()),
                       h->sorted_row, n, reinterpret_cast<uint32_t*>(tmp.get()));
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h->ty_types, tmp, 4 * (size_t)n, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = fail(h, NL_ERR_HIP);
  }
  h->ty_gen++;
  return rc;
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
    DevBuf<uint32_t> bad;
    if (int rc = side_alloc(h, bad, 16)) return rc;
    uint32_t b = 0;
    HIPCHK(h, hipMemsetAsync(bad, 0, 16, s));
    if (n > 0) {
      hipLaunchKernelGGL(k_type_check, dim3((uint32_t)std::max(1, std::min((n + 255) / 256, 8 * h->num_cus))), dim3(256), 0, s, types_dev, n, ntypes, bad);
      HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (b) return fail(h, NL_ERR_ARG);
  }
  // the table, in its buffers where they hold it (a graph the caller captured keeps reading them)
  const bool f32 = h->dtype == NL_F32;
  const size_t thr_bytes = (f32 ? 4 : 8) * (size_t)NL_MAX_TYPES * NL_MAX_TYPES;
  if (!h->ty_types.holds(n))
    if (int rc = swap_alloc(h, h->ty_types, 4 * ((size_t)h->n_max + 16), h->n_max)) return rc;
  if (!h->ty_rc2)
    if (int rc = swap_alloc(h, h->ty_rc2, thr_bytes)) {
      types_clear(h);
      return rc;
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
  if (int rc = filter_reserve(h)) {  // no room for the unfiltered buffers: no table
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
      // (a pair of types the list leaves out, rc_ab = 0, takes rc_force_ab = 0: no entry, no force)
      const bool unlisted = h->ty_rc[k] == 0.0 && rc_force[k] == 0.0;
      if (!std::isfinite(epsilon[k]) || !(sigma[k] > 0) || !std::isfinite(sigma[k]) || !(rc_force[k] > 0 || unlisted) ||
          !(rc_force[k] <= h->ty_rc[k]) || epsilon[k] != epsilon[t] || sigma[k] != sigma[t] || rc_force[k] != rc_force[t])
        return fail(h, NL_ERR_ARG);
    }
  HIPCHK(h, hipSetDevice(h->device));
  constexpr int NT2 = NL_MAX_TYPES * NL_MAX_TYPES;
  const bool f32 = h->dtype == NL_F32;
  const size_t bytes = (f32 ? 4 : 8) * 3 * (size_t)NT2;
  if (!h->lj_par) {
    HIPCHK(h, hipDeviceSynchronize());
    if (int rc = side_alloc(h, h->lj_par, bytes)) return rc;
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

}  // extern "C"
