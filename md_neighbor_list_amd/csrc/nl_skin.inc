// nl_skin.inc -- the Verlet part of the Verlet list (SURVEY.md section 8 f2, "skin distance, rebuild trigger"): a list built
// with cut-off rc (= the physical cut-off + skin) is reused until some particle has moved more than skin / 2 since that
// build.  nl_update_list takes that decision on the device, in stream order, and rebuilds only when the list no longer
// holds -- no host round trip, so that a whole MD step (integrate, update, forces) can be enqueued ahead and replayed
// from a graph.  One update enqueues, on one stream and as one linear chain:
//   k_skin_check   one pass over q and the snapshot of the last performed build; its last block writes the word `go`
//   the build      the build of nl_make_list, every launch of which leaves at entry while go == 0 (gate_closed)
//   k_skin_snap    go == 1: snapshot <- q
//   result copy    the meta words, as after any build (after a skipped update: the last build's, again)
// The build is the one finish() would run again (plan_build's rerun): two-pass binning and every launch of its path, because an
// asynchronous MD loop never calls finish().
// Included at the end of nl_api.hip.

namespace {

// words of h->skin_words
constexpr int SKIN_GO = 0;        // 1: the update builds (every launch of its build reads it)
constexpr int SKIN_OVER = 1;      // some block saw a particle past skin / 2 (zero between updates)
constexpr int SKIN_TICKET = 2;    // blocks of k_skin_check through (zero between updates)
constexpr int SKIN_COUNTERS = 4;  // two uint64: updates, builds they performed
constexpr int SKIN_WORDS = 8;
constexpr int SKIN_THREADS = 256;

// Rule (c) of nl_update_list, per particle: d = q - snap per component in T (round to nearest, no contraction), widened
// to double, folded to the minimum image on the axes of the mask (d -= L rint(d / L)), r2 = (dx^2 + dy^2) + dz^2 in double without
// FMA; the particle is past the skin where !(r2 <= (skin/2)^2), which also holds for NaN.  The OR of that flag over all
// particles decides exactly what "max_i r2 > (skin/2)^2 or any r2 NaN" decides, so no maximum is formed: a block
// ORs its waves' flags and adds at most one atomic.  The last block through (ticket, as in k_bin_bucket) adds the
// host's reasons (`force`) and the status word of the last build, writes go, counts the update, puts its own words
// back to zero and -- go == 1 only -- clears what the build expects cleared (`zero`: meta words and row totals of the
// two-pass binning, which a plain build clears with a memset node).
template <typename T, bool PBC>
__global__ void __launch_bounds__(SKIN_THREADS) k_skin_check(const T* __restrict__ q, const T* __restrict__ snap, int32_t stride,
                                                             int32_t n, double thr, double Lx, double Ly, double Lz, int32_t mask, int32_t force,
                                                             uint32_t* __restrict__ words, const uint32_t* status, int32_t* zero,
                                                             int32_t nzero, double xy, double xz, double yz) {
  __shared__ int32_t last_s;
  __shared__ uint32_t go_s;
  bool past = false;
  for (int32_t i = blockIdx.x * SKIN_THREADS + threadIdx.x; i < n; i += gridDim.x * SKIN_THREADS) {
    T x, y, z, sx, sy, sz;
    load_xyz(q, stride, i, x, y, z);
    load_xyz(snap, stride, i, sx, sy, sz);
    double dx = (double)sub_rn(x, sx), dy = (double)sub_rn(y, sy), dz = (double)sub_rn(z, sz);
    if (PBC && (xy != 0 || xz != 0 || yz != 0)) {  // triclinic (nl_set_box): z, y, x as LAMMPS' minimum_image, rint form
      if (mask & 4) {
        const double k = rint(dz / Lz);
        dz = __dsub_rn(dz, __dmul_rn(k, Lz)), dy = __dsub_rn(dy, __dmul_rn(k, yz)), dx = __dsub_rn(dx, __dmul_rn(k, xz));
      }
      if (mask & 2) {
        const double k = rint(dy / Ly);
        dy = __dsub_rn(dy, __dmul_rn(k, Ly)), dx = __dsub_rn(dx, __dmul_rn(k, xy));
      }
      if (mask & 1) dx = __dsub_rn(dx, __dmul_rn(Lx, rint(dx / Lx)));
    } else if (PBC) {  // (mask: the axes of the minimum image, nl_set_periodic_axes)
      if (mask & 1) dx = __dsub_rn(dx, __dmul_rn(Lx, rint(dx / Lx)));
      if (mask & 2) dy = __dsub_rn(dy, __dmul_rn(Ly, rint(dy / Ly)));
      if (mask & 4) dz = __dsub_rn(dz, __dmul_rn(Lz, rint(dz / Lz)));
    }
    const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
    past |= !(r2 <= thr);
  }
  const int any = __syncthreads_or(past ? 1 : 0);
  if (threadIdx.x == 0) {
    if (any) atomicOr(words + SKIN_OVER, 1u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_s_waitcnt(0);  // the flag is in before the ticket
    last_s = atomicAdd(words + SKIN_TICKET, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last_s) return;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t over = __hip_atomic_load(words + SKIN_OVER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t go = force || over || status[0] != 0u ? 1u : 0u;  // (b): the last build did not succeed
    words[SKIN_GO] = go;
    __hip_atomic_store(words + SKIN_OVER, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(words + SKIN_TICKET, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(words + SKIN_COUNTERS);
    cnt[0] += 1;
    cnt[1] += go;
    go_s = go;
  }
  __syncthreads();  // (status[0] has been read)
  if (go_s)
    for (int32_t k = threadIdx.x; k < nzero; k += SKIN_THREADS) zero[k] = 0;
}

// snapshot <- the caller's positions (input order, q's stride), where the update built
template <typename T>
__global__ void __launch_bounds__(256) k_skin_snap(const T* __restrict__ q, T* __restrict__ snap, int64_t count,
                                                   const uint32_t* __restrict__ gate) {
  if (gate_closed(gate)) return;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) snap[k] = q[k];
}

// The launches of one update on stream s (see the top of this file): the build of arguments a along plan p (made with
// rerun).  force: a reason the host knows (rule (a)).
template <typename T>
int enqueue_update(nl_handle_t h, const BuildArgs& a, const BuildPlan& p, bool force, hipStream_t s) {
  const int32_t n = a.n, stride = a.stride, nrows = h->m[1] * a.mzl;
  const double half = 0.5 * h->skin, thr = half * half;
  const int32_t grid = std::max(1, std::min((n + 4 * SKIN_THREADS - 1) / (4 * SKIN_THREADS), 4 * h->num_cus));
  const T* q = static_cast<const T*>(a.q);
  T* snap = static_cast<T*>(h->snap);
  // (the two-pass binning of the build clears meta words + row totals, which k_skin_check does here; the atomic-rank
  // binning clears histogram + meta words with a gated launch of its own)
  int32_t* zero = reinterpret_cast<int32_t*>(h->status);
  const int32_t nzero = p.binning == BINNING_TWO_PASS ? 32 + nrows : 0;
  // (the box of this update's plan: a changed box forces the build, so with force == 0 it is the box of the snapshot's build)
  const Box& b = p.box;
  // (nl_set_pair_images: no fold -- a particle the caller re-wrapped has moved by a box vector, and the update builds)
  if (h->pbc != 0 && !p.images)
    hipLaunchKernelGGL((k_skin_check<T, true>), dim3(grid), dim3(SKIN_THREADS), 0, s, q, snap, stride, n, thr, b.L[0], b.L[1],
                       b.L[2], h->pbc, force ? 1 : 0, h->skin_words, h->status, zero, nzero, b.xy, b.xz, b.yz);
  else
    hipLaunchKernelGGL((k_skin_check<T, false>), dim3(grid), dim3(SKIN_THREADS), 0, s, q, snap, stride, n, thr, b.L[0], b.L[1],
                       b.L[2], 0, force ? 1 : 0, h->skin_words, h->status, zero, nzero, 0.0, 0.0, 0.0);
  h->gate = h->skin_words + SKIN_GO;
  int rc = enqueue_build<T>(h, a, p, s, nullptr);
  if (!rc) {
    const int64_t count = (int64_t)n * stride;
    const uint32_t sgrid = (uint32_t)std::max<int64_t>(1, std::min<int64_t>((count + 1023) / 1024, 1024));
    hipLaunchKernelGGL(k_skin_snap<T>, dim3(sgrid), dim3(256), 0, s, q, snap, count, h->gate);
    rc = enqueue_result_copy(h, s);
  }
  h->gate = nullptr;
  if (!rc) HIPCHK(h, hipGetLastError());
  return rc;
}

int dispatch_update(nl_handle_t h, const BuildArgs& a, const BuildPlan& p, bool force, hipStream_t s) {
  return h->dtype == NL_F32 ? enqueue_update<float>(h, a, p, force, s) : enqueue_update<double>(h, a, p, force, s);
}

}  // namespace

extern "C" {

int nl_set_skin(nl_handle_t h, double skin) {
  if (!h || !(skin >= 0) || !std::isfinite(skin)) return fail(h, NL_ERR_ARG);
  h->skin = skin;
  h->upd_valid = false;
  return NL_OK;
}

int nl_update_list(nl_handle_t h, const void* q_dev, int32_t q_stride, int32_t n, void* stream, int sync) {
  if (!h) return NL_ERR_ARG;
  if (h->n_max <= 0 && n > 0) return fail(h, NL_ERR_STATE);
  if (n < 0 || n > h->n_max || (q_stride != 3 && q_stride != 4) || (!q_dev && n > 0)) return fail(h, NL_ERR_ARG);
  if (excl_refuses(h, nullptr, n) || (h->ty_types && n != h->ty_n)) return fail(h, NL_ERR_ARG);  // (nl_set_exclusions, nl_set_type_cutoffs)
  if (!tilt_mask_ok(h)) return fail(h, NL_ERR_STATE);  // (nl_set_box: a tilt needs both of its axes periodic)
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIPCHK(h, hipStreamIsCapturing(s, &cap));
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (!capturing)  // (again, if an allocation failed since a table or the flag was set)
    if (int rc = stage_reserve(h)) return rc;
  // (a): what forces a build before any particle is looked at -- no list of an update to keep (a setter, nl_resort or
  // another kind of build since, the host has seen the last build fail), or other positions
  const bool force = !h->upd_valid || q_dev != h->upd_q || q_stride != h->upd_stride || n != h->upd_n || (!h->pending && !h->built);
  // the caller is capturing its stream: plain launches only -- nothing allocated, nothing waited for, no build that the
  // host would have to decide at every replay
  if (capturing && (force || (h->pending && h->last_stream != s))) return fail(h, NL_ERR_STATE);
  if (h->pending) {  // as nl_make_list: stream order keeps an update behind the previous build on the same stream
    if (h->last_stream != s) HIPCHK(h, hipStreamSynchronize(h->last_stream));
    h->pending = false;
  }
  if (force) {
    const size_t need = (h->dtype == NL_F32 ? 4 : 8) * 4 * ((size_t)h->n_max + 1);
    if (h->snap.bytes() < need)
      if (int rc = dev_alloc(h, h->snap, need)) return rc;
    if (!h->skin_words) {
      if (int rc = dev_alloc(h, h->skin_words, sizeof(uint32_t) * SKIN_WORDS)) return rc;
      HIPCHK(h, hipMemset(h->skin_words, 0, sizeof(uint32_t) * SKIN_WORDS));
    }
  }
  h->built = false;
  h->t_valid = false;
  h->n = n, h->n_rows = n;
  const BuildArgs a{q_dev, q_stride, nullptr, n, n, 0, 0, h->m[2], 0};
  const BuildPlan p = plan_for(h, a, PART_ALL, true);  // (an update's build: two-pass binning, every launch)
  if (h->use_graph && !capturing && !force) {
    // the same graph as nl_make_list's (one per argument set), keyed also on the update and its skin; a forced update
    // runs as plain launches and the next one captures
    adopt_build(h, a, p);
    const GraphKey key{a, p, h->capacity, h->buffers_epoch, h->ex_gen, h->ty_gen, 1, h->skin};
    if (int rc = graph_launch(h, key, s, [&](hipStream_t cs) { return dispatch_update(h, a, p, false, cs); })) return rc;
  } else {
    if (int rc = dispatch_update(h, a, p, force, s)) return rc;
  }
  h->upd_valid = true, h->last_update = true;
  h->upd_q = q_dev, h->upd_stride = q_stride, h->upd_n = n;
  h->last_stream = s;
  h->pending = true;
  if (sync) return finish(h, true);
  return NL_OK;
}

int nl_get_update_stats(nl_handle_t h, int64_t stats[2]) {
  if (!h || !stats) return fail(h, NL_ERR_ARG);
  stats[0] = stats[1] = 0;
  if (!h->skin_words) return NL_OK;
  HIPCHK(h, hipSetDevice(h->device));
  // (the whole device: updates the caller captured into a graph of its own run on whichever stream it replays them)
  HIPCHK(h, hipDeviceSynchronize());
  unsigned long long c[2] = {0, 0};
  HIPCHK(h, hipMemcpy(c, h->skin_words + SKIN_COUNTERS, sizeof(c), hipMemcpyDeviceToHost));
  stats[0] = (int64_t)c[0], stats[1] = (int64_t)c[1];
  return NL_OK;
}

}  // extern "C"
