// nl_exclude.inc -- excluded pairs (nl_set_exclusions): the bonded partners of a molecular model (1-2, 1-3 pairs) left out of
// the non-bonded list when it is built, so that the list is filtered once per build and every consumer sees the same list.
//   The table   a symmetric CSR over input-order particle ids, per-row ascending, without duplicates; built on the device
//               from the caller's pairs (k_excl_degree .. k_excl_pack), relabelled by the first nl_resort after a build.
//               Or (nl_set_exclusions_global) the same CSR over the ids the list stores, [0, n_ids): the caller's names,
//               never relabelled, the same on every rank of a decomposed run; 4 bytes of offsets per global id.
//   The stage   behind the search of a build, on its stream: the search writes the unfiltered offsets and list into
//               kp_pre / list_pre (search_kp, search_list); k_excl_count counts what each row keeps into `count`, the
//               row scan turns that into key_pointer (its total into the meta words, META_KEPT), k_excl_compact copies
//               the kept entries into `list`.  A wave per row; the row's excluded ids are broadcast with readlane, or
//               binary-searched where a row has more than EXCL_BCAST of them.  Every kernel takes the update's gate.
//   The row's id  indexes the table: the row number (whole builds, slab builds without ids: the instances of the
//               input-row table), or with a global table gid[row] or the w component of the caller's positions
//               (ExclIds, EXCL_ID_*): one dependent load per row.  An id outside [0, n_ids) flags ST_ID_RANGE.
// Builds without a table launch none of this and use the buffers they always used.
// Included at the end of nl_api.hip; the pieces it shares with the other stages: nl_stage.hpp.

namespace {

constexpr int EXCL_BCAST = 32;  // rows with up to this many excluded ids compare against registers; more: binary search

// Is v (a partner of the row) one of the row's excluded ids?  exid: lane l holds ids[xb + l] for l < ne (<= EXCL_BCAST).
__device__ __forceinline__ bool excl_hit(int32_t v, int32_t exid, int32_t ne, const int32_t* __restrict__ ids, int32_t xb) {
  if (ne > EXCL_BCAST) return sorted_contains(ids, xb, ne, v);
  bool hit = false;
  for (int32_t t = 0; t < ne; t++) hit |= v == __builtin_amdgcn_readlane(exid, t);  // (ne is uniform)
  return hit;
}

template <typename OFF> struct ExclArgs {
  const OFF* __restrict__ kp_pre;  // the unfiltered offsets and list
  const int32_t* __restrict__ list_pre;
  int32_t n_rows;
  int64_t capacity;
  const int32_t* __restrict__ ex_off;  // the table
  const int32_t* __restrict__ ex_ids;
  const uint32_t* __restrict__ gate;
};

// Where a row's id comes from (compile-time): the row number, or for a global table the caller's id of the row.
enum { EXCL_ID_ROW = 0, EXCL_ID_GID = 1, EXCL_ID_W32 = 2, EXCL_ID_W64 = 3 };
struct ExclIds {
  const void* __restrict__ src;  // EXCL_ID_GID: int32 gid[n_rows]; EXCL_ID_W32 / _W64: the positions, stride 4, id bits in w
  int32_t n_ids;                 // ids of the table: a row id outside [0, n_ids) fails the build
  uint32_t* __restrict__ status;
};

// The id of a row, wave-uniform (the row is).  -1: outside the table (flagged once per row, by the count pass).
template <int IDS, bool FLAG> __device__ __forceinline__ int32_t excl_row_id(const ExclIds& x, int32_t row, int lane) {
  int32_t id;
  if constexpr (IDS == EXCL_ID_GID) id = static_cast<const int32_t*>(x.src)[row];
  else if constexpr (IDS == EXCL_ID_W32) id = __float_as_int(static_cast<const float*>(x.src)[(size_t)row * 4 + 3]);
  else id = (int32_t)__double_as_longlong(static_cast<const double*>(x.src)[(size_t)row * 4 + 3]);
  id = __builtin_amdgcn_readfirstlane(id);
  if ((uint32_t)id < (uint32_t)x.n_ids) return id;
  if (FLAG && lane == 0) atomicOr(x.status, ST_ID_RANGE);
  return -1;
}

// Both passes of the stage, a wave per row.  Count: count[row] = entries of the unfiltered row that the table keeps; rows
// without exclusions do not read the list.  COMPACT: list[kp[row] ...] = the kept entries in their order (ballot + mbcnt).
// (Entries at or past the list capacity were never written: an overflowed build fails, and they are only not read.)
template <typename OFF, bool COMPACT, int IDS = EXCL_ID_ROW>
__device__ __forceinline__ void excl_pass(const ExclArgs<OFF>& a, int32_t* __restrict__ count, const OFF* __restrict__ kp,
                                          int32_t* __restrict__ list, const ExclIds& x = ExclIds{}) {
  if (gate_closed(a.gate)) return;  // (nl_update_list: no build this time)
  const int lane = threadIdx.x & 63;
  const int32_t waves = gridDim.x * (STAGE_THREADS / WAVE);
  for (int32_t row = blockIdx.x * (STAGE_THREADS / WAVE) + (threadIdx.x >> 6); row < a.n_rows; row += waves) {
    const int64_t b = (int64_t)a.kp_pre[row], e = (int64_t)a.kp_pre[row + 1];
    const int64_t end = e < a.capacity ? e : a.capacity;
    int32_t xb, ne;
    if constexpr (IDS == EXCL_ID_ROW) {
      xb = a.ex_off[row], ne = a.ex_off[row + 1] - xb;
    } else {  // (a row outside the table keeps everything; its build fails)
      const int32_t id = excl_row_id<IDS, !COMPACT>(x, row, lane);
      xb = id < 0 ? 0 : a.ex_off[id], ne = id < 0 ? 0 : a.ex_off[id + 1] - xb;
    }
    int64_t kept = e - b, dst = 0;
    if constexpr (COMPACT) dst = (int64_t)kp[row];
    if (ne == 0) {
      if constexpr (COMPACT)
        for (int64_t k = b + lane; k < end; k += WAVE) {
          const int64_t d = dst + (k - b);
          if (d < a.capacity) list[d] = a.list_pre[k];
        }
    } else {
      const int32_t exid = lane < ne && ne <= EXCL_BCAST ? a.ex_ids[xb + lane] : -1;
      for (int64_t k = b + lane; k - lane < end; k += WAVE) {
        const int32_t v = k < end ? a.list_pre[k] : -1;
        const bool hit = excl_hit(v, exid, ne, a.ex_ids, xb);  // (no short cut: readlane in it)
        if constexpr (COMPACT) {
          const bool keep = !hit & (k < end);
          const uint64_t mask = __ballot(keep);
          const int64_t d = dst + lanes_below(mask);
          if (keep && d < a.capacity) list[d] = v;
          dst += __builtin_popcountll(mask);
        } else {
          kept -= __builtin_popcountll(__ballot(hit & (k < end)));
        }
      }
    }
    if (!COMPACT && lane == 0) count[row] = (int32_t)kept;
  }
}

template <typename OFF> __global__ void __launch_bounds__(STAGE_THREADS) k_excl_count(ExclArgs<OFF> a, int32_t* __restrict__ count) {
  excl_pass<OFF, false>(a, count, nullptr, nullptr);
}
template <typename OFF>
__global__ void __launch_bounds__(STAGE_THREADS) k_excl_compact(ExclArgs<OFF> a, const OFF* __restrict__ kp, int32_t* __restrict__ list) {
  excl_pass<OFF, true>(a, nullptr, kp, list);
}

// The same two passes with the table indexed by the caller's id of the row (a global table on a build with ids).
template <typename OFF> struct ExclIdArgs {
  ExclArgs<OFF> a;
  ExclIds x;
};
template <typename OFF, int IDS> __global__ void __launch_bounds__(STAGE_THREADS) k_excl_count_id(ExclIdArgs<OFF> a, int32_t* __restrict__ count) {
  excl_pass<OFF, false, IDS>(a.a, count, nullptr, nullptr, a.x);
}
template <typename OFF, int IDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_excl_compact_id(ExclIdArgs<OFF> a, const OFF* __restrict__ kp, int32_t* __restrict__ list) {
  excl_pass<OFF, true, IDS>(a.a, nullptr, kp, list, a.x);
}

// (declared at the top of nl_api.hip)  The build's ids are its rows (every build of an input-row table; a global table
// on a build without caller ids, whose rows the entry point has checked against n_ids): the row-indexed instances.
int launch_exclude(nl_handle_t h, int32_t n_rows, hipStream_t s) {
  return dispatch_t_off(h, [&](auto, auto off) -> int {
    using OFF = decltype(off);
    const ExclArgs<OFF> a = {static_cast<const OFF*>(h->kp_pre), h->list_pre, n_rows, h->capacity, h->ex_off, h->ex_ids, h->gate};
    if (!h->args.gid) return launch_passes<OFF>(h, n_rows, n_rows, s, a, k_excl_count<OFF>, k_excl_compact<OFF>);
    const bool in_w = h->args.gid == NL_GID_IN_W;
    const ExclIdArgs<OFF> ax = {a, ExclIds{in_w ? h->args.q : static_cast<const void*>(h->args.gid), h->ex_n, h->status}};
    auto launch = [&](auto ids) {
      constexpr int IDS = decltype(ids)::value;
      return launch_passes<OFF>(h, n_rows, n_rows, s, ax, k_excl_count_id<OFF, IDS>, k_excl_compact_id<OFF, IDS>);
    };
    if (!in_w) return launch(std::integral_constant<int, EXCL_ID_GID>());
    if (h->dtype == NL_F32) return launch(std::integral_constant<int, EXCL_ID_W32>());
    return launch(std::integral_constant<int, EXCL_ID_W64>());
  });
}

// ------------------------------------------------------------------------------------------- the table, on the device
// deg[a]++, deg[b]++ for every valid pair; an invalid one (out of [0, n), or a == b) sets *bad.
__global__ void __launch_bounds__(256) k_excl_degree(const int32_t* __restrict__ pairs, int64_t np, int32_t n, int32_t* __restrict__ deg,
                                                     uint32_t* __restrict__ bad) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < np; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t a = pairs[2 * e], b = pairs[2 * e + 1];
    if (a < 0 || a >= n || b < 0 || b >= n || a == b) {
      atomicOr(bad, 1u);
      continue;
    }
    atomicAdd(&deg[a], 1);
    atomicAdd(&deg[b], 1);
  }
}

// Both directions of every pair into the rows of off[] (cursor[] zero on entry), in no particular order.
__global__ void __launch_bounds__(256) k_excl_scatter(const int32_t* __restrict__ pairs, int64_t np, const int32_t* __restrict__ off,
                                                      int32_t* __restrict__ cursor, int32_t* __restrict__ ids) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < np; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t a = pairs[2 * e], b = pairs[2 * e + 1];
    ids[off[a] + atomicAdd(&cursor[a], 1)] = b;
    ids[off[b] + atomicAdd(&cursor[b], 1)] = a;
  }
}

// A wave per row: every entry goes to its rank in the row (ties by position), so the row comes out ascending.  The rank
// is counted against the whole row: m^2 / 64 steps, a few for bonded rows (and 625 for a hub of 200).
__global__ void __launch_bounds__(256) k_excl_sort_rows(const int32_t* __restrict__ off, const int32_t* __restrict__ in, int32_t n,
                                                        int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int32_t waves = gridDim.x * 4;
  for (int32_t row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += waves) {
    const int32_t b = off[row], m = off[row + 1] - b;
    for (int32_t k = lane; k - lane < m; k += WAVE) {
      const int32_t v = k < m ? in[b + k] : 0;
      int32_t rank = 0;
      for (int32_t j = 0; j < m; j++) {
        const int32_t u = in[b + j];  // (uniform address)
        rank += u < v || (u == v && j < k);
      }
      if (k < m) out[b + rank] = v;
    }
  }
}

// cnt[row] = distinct ids of a sorted row
__global__ void __launch_bounds__(256) k_excl_distinct(const int32_t* __restrict__ off, const int32_t* __restrict__ ids, int32_t n,
                                                       int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int32_t waves = gridDim.x * 4;
  for (int32_t row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += waves) {
    const int32_t b = off[row], m = off[row + 1] - b;
    int32_t c = 0;
    for (int32_t k = lane; k - lane < m; k += WAVE) {
      const bool first = k < m && (k == 0 || ids[b + k] != ids[b + k - 1]);
      c += __builtin_popcountll(__ballot(first));
    }
    if (lane == 0) cnt[row] = c;
  }
}

// The distinct ids of every sorted row at the row's new offset.
__global__ void __launch_bounds__(256) k_excl_pack(const int32_t* __restrict__ off, const int32_t* __restrict__ ids, const int32_t* __restrict__ off_new,
                                                   int32_t n, int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int32_t waves = gridDim.x * 4;
  for (int32_t row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += waves) {
    const int32_t b = off[row], m = off[row + 1] - b;
    int32_t dst = off_new[row];
    for (int32_t k = lane; k - lane < m; k += WAVE) {
      const bool first = k < m && (k == 0 || ids[b + k] != ids[b + k - 1]);
      const uint64_t mask = __ballot(first);
      if (first) out[dst + (int32_t)lanes_below(mask)] = ids[b + k];
      dst += __builtin_popcountll(mask);
    }
  }
}

// inv[order[s]] = s
__global__ void __launch_bounds__(256) k_excl_inverse(const int32_t* __restrict__ order, int32_t n, int32_t* __restrict__ inv) {
  const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) inv[order[s]] = s;
}

// The table's entries as pairs (inv[row], inv[id]) -- both directions, which the set-up merges again.
__global__ void __launch_bounds__(256) k_excl_relabel(const int32_t* __restrict__ off, const int32_t* __restrict__ ids, const int32_t* __restrict__ inv,
                                                      int32_t n, int32_t* __restrict__ pairs) {
  const int32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const int32_t r = inv[row];
  for (int32_t k = off[row]; k < off[row + 1]; k++) {
    pairs[2 * (int64_t)k] = r;
    pairs[2 * (int64_t)k + 1] = inv[ids[k]];
  }
}

uint32_t excl_grid(int64_t items, int32_t per_block, int32_t max_blocks) {
  return (uint32_t)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, max_blocks));
}

// Builds a table from np pairs on the handle's stream and makes it the handle's; validate: pairs out of range or with
// i == j are NL_ERR_ARG and leave the old table in place.  global: the rows are ids of the list (nl_set_exclusions_global),
// as many as the caller names -- more than the handle's scan holds blocks for take a look-back array of their own.
// Synchronous.
int excl_build(nl_handle_t h, const int32_t* pairs, int64_t np, int32_t n, bool validate, bool global) {
  if (2 * np > 2147483000LL) return fail(h, NL_ERR_ARG);
  hipStream_t s = h->own_stream;
  const size_t rows = (size_t)n + 32, ents = 2 * (size_t)np + 16;
  DevBuf<int32_t> deg, off_raw, raw, srt, off_new;  // (freed on every way out)
  DevBuf<uint32_t> bad;
  DevBuf<uint64_t> look;
  const int32_t scan_nb = (int32_t)(((int64_t)n + SCAN_BLOCK - 1) / SCAN_BLOCK);
  auto scan = [&](const int32_t* in, int32_t* out) -> int {
    if (!look) return launch_scan(h, in, n, out, h->totals + 2, s);
    hipLaunchKernelGGL(k_scan_chained<int32_t>, dim3(scan_nb), dim3(SCAN_THREADS), 0, s, in, (int64_t)n, look, scan_nb, h->totals + 2, out, h->status,
                       static_cast<uint32_t*>(nullptr), static_cast<const uint32_t*>(nullptr));
    return NL_OK;
  };
  int rc;
  if ((rc = side_alloc(h, deg, 4 * rows)) || (rc = side_alloc(h, off_raw, 4 * rows)) || (rc = side_alloc(h, raw, 4 * ents)) ||
      (rc = side_alloc(h, srt, 4 * ents)) || (rc = side_alloc(h, off_new, 4 * rows)) || (rc = side_alloc(h, bad, 16)))
    return rc;
  if (n > SCAN_SMALL_MAX && scan_nb > h->scan_blocks) {  // (k_scan_chained leaves its array zero again)
    if ((rc = side_alloc(h, look, 8 * ((size_t)scan_nb + 1)))) return rc;
    HIPCHK(h, hipMemsetAsync(look, 0, 8 * ((size_t)scan_nb + 1), s));
  }
  HIPCHK(h, hipMemsetAsync(deg, 0, 4 * rows, s));
  HIPCHK(h, hipMemsetAsync(bad, 0, 16, s));
  const uint32_t pgrid = excl_grid(np, 256, 8 * h->num_cus), rgrid = excl_grid(n, 4, 16 * h->num_cus);
  if (np > 0) hipLaunchKernelGGL(k_excl_degree, dim3(pgrid), dim3(256), 0, s, pairs, np, n, deg, bad);
  HIPCHK(h, hipGetLastError());
  if (validate) {
    uint32_t b = 0;
    HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (b) return fail(h, NL_ERR_ARG);
  }
  if ((rc = scan(deg, off_raw))) return rc;
  HIPCHK(h, hipMemsetAsync(deg, 0, 4 * rows, s));
  if (np > 0) hipLaunchKernelGGL(k_excl_scatter, dim3(pgrid), dim3(256), 0, s, pairs, np, off_raw, deg, raw);
  if (n > 0) {
    hipLaunchKernelGGL(k_excl_sort_rows, dim3(rgrid), dim3(256), 0, s, off_raw, raw, n, srt);
    hipLaunchKernelGGL(k_excl_distinct, dim3(rgrid), dim3(256), 0, s, off_raw, srt, n, deg);
  }
  if ((rc = scan(deg, off_new))) return rc;
  if (n > 0) hipLaunchKernelGGL(k_excl_pack, dim3(rgrid), dim3(256), 0, s, off_raw, srt, off_new, n, raw);
  HIPCHK(h, hipGetLastError());
  int32_t entries = 0;
  HIPCHK(h, hipMemcpyAsync(&entries, off_new + n, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (h->ex_ids && 4 * ((size_t)n + 1) <= h->ex_off.bytes() && 4 * (size_t)entries <= h->ex_ids.bytes()) {
    // into the buffers the table has: a graph the caller captured (an update, forces) keeps finding it there -- a
    // relabel always fits (same n, same entries)
    HIPCHK(h, hipMemcpyAsync(h->ex_off, off_new, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->ex_ids, raw, 4 * (size_t)entries, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
  } else {  // the new table replaces the old one
    h->buffers_epoch++;
    h->ex_off.adopt(off_new), h->ex_ids.adopt(raw);
  }
  h->ex_n = n;
  h->ex_global = global;
  h->ex_unique = entries / 2;
  h->ex_gen++;
  return NL_OK;
}

void excl_clear(nl_handle_t h) {
  h->ex_off.release(), h->ex_ids.release();
  if (!h->ty_types) filter_release(h);
  h->ex_n = 0, h->ex_unique = 0;
  h->ex_global = false;
  h->ex_gen++;
  h->buffers_epoch++;
}

// (declared at the top of nl_api.hip) The table in the cell order of the last build: (a, b) -> (inv[a], inv[b]).
int excl_relabel(nl_handle_t h) {
  const int32_t n = h->ex_n;
  const int64_t entries = 2 * h->ex_unique;
  DevBuf<int32_t> inv, pairs;
  hipStream_t s = h->own_stream;
  HIPCHK(h, hipDeviceSynchronize());  // (replays of a graph the caller captured may still read the table)
  if (int rc = side_alloc(h, inv, 4 * ((size_t)n + 16))) return rc;
  if (int rc = side_alloc(h, pairs, 8 * ((size_t)entries + 16))) return rc;
  if (n == 0) return NL_OK;
  hipLaunchKernelGGL(k_excl_inverse, dim3((n + 255) / 256), dim3(256), 0, s, h->sorted_row, n, inv);
  hipLaunchKernelGGL(k_excl_relabel, dim3((n + 255) / 256), dim3(256), 0, s, h->ex_off, h->ex_ids, inv, n, pairs);
  if (hipGetLastError() != hipSuccess) return fail(h, NL_ERR_HIP);
  return excl_build(h, pairs, entries, n, false, false);
}

// nl_set_exclusions (rows: n <= n_max) and nl_set_exclusions_global (ids: as many as the caller names; the row loops
// count in int32, so below 2^31 - 647): one table per handle, of the kind set last.
int excl_set(nl_handle_t h, const int32_t* pairs_dev, int64_t n_pairs, int32_t n, bool global) {
  if (!h || n_pairs < 0) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  if (n_pairs == 0 || !pairs_dev) {
    if (h->ex_ids) excl_clear(h);
    h->upd_valid = false;
    return NL_OK;
  }
  if (n < 0 || (global ? n > 2147483000 : n > h->n_max)) return fail(h, NL_ERR_ARG);
  if (!h->totals) return fail(h, NL_ERR_STATE);  // (the set-up scans with the handle's buffers: nl_initialize first)
  HIPCHK(h, hipDeviceSynchronize());  // (the caller's pairs may come from any stream)
  if (int rc = excl_build(h, pairs_dev, n_pairs, n, true, global)) return rc;
  h->upd_valid = false;
  if (int rc = filter_reserve(h)) {  // no room for the pre-exclusion buffers: no table
    excl_clear(h);
    return rc;
  }
  return NL_OK;
}

}  // namespace

extern "C" {

int nl_set_exclusions(nl_handle_t h, const int32_t* pairs_dev, int64_t n_pairs, int32_t n) {
  return excl_set(h, pairs_dev, n_pairs, n, false);
}

int nl_set_exclusions_global(nl_handle_t h, const int32_t* pairs_dev, int64_t n_pairs, int32_t n_ids) {
  return excl_set(h, pairs_dev, n_pairs, n_ids, true);
}

int nl_get_exclusions(nl_handle_t h, const int32_t** offsets_dev, const int32_t** ids_dev, int32_t* n, int64_t* n_unique) {
  if (!h) return NL_ERR_ARG;
  if (!h->ex_ids) return fail(h, NL_ERR_STATE);
  if (offsets_dev) *offsets_dev = h->ex_off;
  if (ids_dev) *ids_dev = h->ex_ids;
  if (n) *n = h->ex_n;
  if (n_unique) *n_unique = h->ex_unique;
  return NL_OK;
}

}  // extern "C"
