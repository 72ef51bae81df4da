// nl_stage.hpp -- what the stages behind the search share: the filter stage (nl_exclude.inc,
// nl_types.inc), the image stage and nl_pair_vectors (nl_images.inc) and the Lennard-Jones consumer (nl_consumer.inc).
//   wave helpers   shfl_t, lanes_below, wave_sum
//   the chunk      a wave takes STAGE_ROWS consecutive rows of a CSR at once: row_chunk, chunk_pick, chunk_row
//   the segment    sorted_contains
//   the frame      particle_frame: a particle's cell faces and wraps as the binning decided them, the 16-bit code the
//                  image stage stores; face_w: the face a partner is reached through
// Every rule here is part of the build's arithmetic contract (which image an entry was tested at): stated once.
// Included by nl_api.hip in front of the .inc files.
#pragma once

#include "nl_kernels.hpp"

namespace nl {

constexpr int STAGE_THREADS = 256;  // block of every stage kernel: 4 waves

// ---------------------------------------------------------------------------------------------------- wave helpers
template <typename T> __device__ __forceinline__ T shfl_t(T v, int src) {
  if constexpr (sizeof(T) == 4) {
    return __int_as_float(__shfl(__float_as_int(v), src, WAVE));
  } else {
    const int lo = __shfl(__double2loint(v), src, WAVE), hi = __shfl(__double2hiint(v), src, WAVE);
    return __hiloint2double(hi, lo);
  }
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------- the chunk
constexpr int STAGE_ROWS = 8;  // rows a wave takes at once (a row of the cfg-2 half list holds ~75 entries)

// The rows [r0, r0 + nr) of a wave's chunk: their entries are contiguous in the list.  Everything here is uniform.
struct RowChunk {
  int64_t beg[STAGE_ROWS + 1];  // first entry of every row; rows past nr begin at the chunk's end
  int64_t b, e;                 // the chunk's entries [b, e), within the list's capacity
  int32_t nr;
};

template <typename OFF>
__device__ __forceinline__ void row_chunk(const OFF* __restrict__ kp, int32_t n_rows, int64_t capacity, int32_t r0, int lane, RowChunk& r) {
  r.nr = min(STAGE_ROWS, n_rows - r0);
  const int64_t v = (int64_t)kp[r0 + min(lane, r.nr)];
#pragma unroll
  for (int t = 0; t <= STAGE_ROWS; t++) {
    const int src = min(t, r.nr);
    r.beg[t] = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int32_t)((uint64_t)v >> 32), src) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int32_t)v, src));
  }
  r.b = max(r.beg[0], (int64_t)0);
  r.e = min(r.beg[STAGE_ROWS], capacity);  // (entries past the capacity were never written: such a build fails, and they are only not read)
}

// v[t] of the local row t that entry k of the chunk lies in (k >= r.b; an entry past the chunk's end gives the last row).
// A list behind int32 offsets is compared in 32 bits, relative to the chunk's first entry.
template <typename OFF, typename V>
__device__ __forceinline__ V chunk_pick(const RowChunk& r, int64_t k, const V (&v)[STAGE_ROWS]) {
  V out = v[0];
  if constexpr (sizeof(OFF) == 4) {
    const uint32_t rel = (uint32_t)(k - r.beg[0]);
#pragma unroll
    for (int t = 1; t < STAGE_ROWS; t++) out = rel >= (uint32_t)(r.beg[t] - r.beg[0]) ? v[t] : out;
  } else {
#pragma unroll
    for (int t = 1; t < STAGE_ROWS; t++) out = k >= r.beg[t] ? v[t] : out;
  }
  return out;
}

// The local row of entry k: the lane that holds what a stage keeps per row (fetched with shfl_t / __shfl).
template <typename OFF> __device__ __forceinline__ int32_t chunk_row(const RowChunk& r, int64_t k) {
  constexpr int32_t rows[STAGE_ROWS] = {0, 1, 2, 3, 4, 5, 6, 7};
  return chunk_pick<OFF>(r, k, rows);
}

// ----------------------------------------------------------------------------------------------------- the segment
// Is v one of the ids of the sorted segment ids[xb, xb + ne)?
__device__ __forceinline__ bool sorted_contains(const int32_t* __restrict__ ids, int32_t xb, int32_t ne, int32_t v) {
  int32_t lo = xb, hi = xb + ne;  // first id >= v
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (ids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < xb + ne && ids[lo] == v;
}

// ------------------------------------------------------------------------------------------------------- the frame
// A particle as the search saw it, in 16 bits: bit d = its cell is the first along axis d, bit 3 + d = the last (axes of
// the mask only), bits 6 + 2d .. 7 + 2d the wrap n_d + 1 that local_cell decides from the input coordinate.
constexpr uint32_t FRAME_NONE = 1u << 6 | 1u << 8 | 1u << 10;  // no faces, no wraps
constexpr uint32_t FRAME_FACES = 63u;

// Runs local_cell once.  shift: where given, receives the stored image's shift (the caller adds it on the axes of the
// mask, as the binning does); a rejected particle leaves it alone and gives FRAME_NONE (its build fails: neither matters).
template <typename T> __device__ __forceinline__ uint32_t particle_frame(const Grid<T>& g, T x, T y, T z, T* shift = nullptr) {
  int32_t lz = 0, row = 0, wrap[3] = {0, 0, 0};
  const int32_t c = local_cell(g, x, y, z, &lz, &row, shift, wrap);
  if (c < 0) return FRAME_NONE;
  const int32_t ci[3] = {c - row * g.m[0], row - lz * g.m[1], lz};
  uint32_t v = 0;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    if ((g.pbc >> d) & 1) v |= (ci[d] == 0 ? 1u : 0u) << d | (ci[d] == g.m[d] - 1 ? 8u : 0u) << d;
    v |= (uint32_t)(wrap[d] + 1) << (6 + 2 * d);
  }
  return v;
}

// w_ij along axis d, from the frames of the row (fi) and of the partner (fj): the face of the i-cell's row of cells that
// the stencil reached the partner through (segment_cells).  -1 where the row's cell is the first and the partner's the
// last (the low face), +1 the other way round, else 0 (m >= 3: never both).  The partner is shifted by
// S(w) = w_a a + w_b b + w_c c (lattice_shift): -+L_d in an orthogonal box.
__device__ __forceinline__ int32_t face_w(uint32_t fi, uint32_t fj, int d) {
  const uint32_t lo_i = (fi >> d) & 1u, hi_i = (fi >> (3 + d)) & 1u;
  const uint32_t lo_j = (fj >> d) & 1u, hi_j = (fj >> (3 + d)) & 1u;
  return (lo_i & hi_j) ? -1 : (hi_i & lo_j) ? 1 : 0;
}

}  // namespace nl
