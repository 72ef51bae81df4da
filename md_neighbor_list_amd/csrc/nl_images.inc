// nl_images.inc -- the periodic image of every entry of the list (nl_set_pair_images) and its consumer (nl_pair_vectors).
//   The rule    include/nl_hip.h: s = n_j + w_ij - n_i, with n the wraps local_cell decides from the input coordinate and w
//               the faces through which the stencil of i's cell reaches j's cell (segment_cells; face_w of nl_stage.hpp states it).
//   The stage   at the very end of a build, behind the filter stage where there is one, on the build's stream:
//               k_image_codes   one thread per particle runs local_cell once and writes its 16-bit frame (particle_frame:
//                               faces and wraps).  2 bytes a particle: the table of a million particles stays in one
//                               XCD's L2.
//               k_pair_images   a wave takes a chunk of STAGE_ROWS consecutive rows of the final key_pointer / list at
//                               once (row_chunk); per entry one 4-byte read, one 2-byte gather of code[j] and one
//                               4-byte vector store of {s_a, s_b, s_c, 0}, coalesced along the list.  No position is read
//                               and local_cell is not run per entry.  The gather is what costs (a cache line per entry
//                               where ids are not spatially ordered), and most builds need little of it: k_image_codes
//                               raises a word when any particle was wrapped; while it is 0 every n is 0, s = w_ij, and
//                               an entry of a row whose cell touches no periodic face is 0 without looking at j.  The
//                               last block of k_pair_images through puts the word back (a ticket, as in k_bin_bucket).
//               The open box (mask 0) has no images: k_zero_images clears the entries of the list.
//               Every kernel takes the update's gate.
//   The consumer  k_pair_vectors: out[k] = {dx, dy, dz, r2} of entry k at its image, the same walk with the row positions
//               held by the lanes.
// Builds with the flag off launch none of this.  Included at the end of nl_api.hip.

namespace {

constexpr int IMG_UNROLL = 4;  // entries a lane keeps in flight
// words of h->img_words (IMG_WORDS of them, nl_api.hip): both zero between builds
constexpr int IMG_WRAPPED = 0;  // some particle of the build has a wrap (k_image_codes)
constexpr int IMG_TICKET = 1;   // blocks of k_pair_images through

template <typename T>
__global__ void __launch_bounds__(STAGE_THREADS) k_image_codes(Grid<T> g, const T* __restrict__ q, int32_t stride, int32_t n,
                                                            uint16_t* __restrict__ code, uint32_t* __restrict__ words) {
  if (gate_closed(g.gate)) return;  // (nl_update_list: no build this time)
  bool wrapped = false;
  for (int32_t i = blockIdx.x * STAGE_THREADS + threadIdx.x; i < n; i += gridDim.x * STAGE_THREADS) {
    T x, y, z;
    load_xyz(q, stride, i, x, y, z);
    const uint32_t v = particle_frame(g, x, y, z);  // (a rejected particle fails its build: its code does not matter)
    wrapped |= (v & ~FRAME_FACES) != FRAME_NONE;
    code[i] = (uint16_t)v;
  }
  if (__ballot(wrapped) != 0ull && (threadIdx.x & 63) == 0) atomicOr(words + IMG_WRAPPED, 1u);
}

// {s_a, s_b, s_c, 0} as bytes of one word, from the codes of the row (ci) and of the partner (cj): the three axes at
// once, one byte each -- the byte-parallel form of s_d = n_j + face_w(ci, cj, d) - n_i (nl_stage.hpp).  Per byte
// (n_j + 1) + [hi_i & lo_j] + 3 - (n_i + 1) - [lo_i & hi_j] = s + 3 lies in 0..6: no borrow crosses a byte; the last
// line takes the 3 off again inside each byte.
__device__ __forceinline__ uint32_t image_word(uint32_t ci, uint32_t cj) {
  constexpr uint32_t BITS = 1u | 1u << 7 | 1u << 14, WRAPS = 1u | 1u << 6 | 1u << 12;  // (bit d -> byte d; field d -> byte d)
  const uint32_t lo_i = ((ci & 7u) * BITS) & 0x010101u, hi_i = (((ci >> 3) & 7u) * BITS) & 0x010101u;
  const uint32_t lo_j = ((cj & 7u) * BITS) & 0x010101u, hi_j = (((cj >> 3) & 7u) * BITS) & 0x010101u;
  const uint32_t n_i = (((ci >> 6) & 63u) * WRAPS) & 0x030303u, n_j = (((cj >> 6) & 63u) * WRAPS) & 0x030303u;
  const uint32_t t = (n_j + (hi_i & lo_j) + 0x030303u) - (n_i + (lo_i & hi_j));
  return ((t | 0x808080u) - 0x030303u) ^ 0x808080u;
}

// The entries of one chunk.  ALL: some particle of the build was wrapped, every entry looks at its partner (the list is
// read first, the rows are found while the gathers are in flight).  Else every n is 0 and s = w_ij: an entry of a row
// whose cell touches no periodic face is 0, and neither the list nor the partner's code is read for it.
template <typename OFF, bool ALL>
__device__ __forceinline__ void image_chunk(const RowChunk& r, const uint32_t (&rc)[STAGE_ROWS], int lane, const int32_t* __restrict__ list,
                                            int32_t n, const uint16_t* __restrict__ code, uint32_t* __restrict__ images) {
  for (int64_t k0 = r.b + lane; k0 - lane < r.e; k0 += IMG_UNROLL * WAVE) {
    int32_t j[IMG_UNROLL];
    uint32_t ci[IMG_UNROLL], cj[IMG_UNROLL];
#pragma unroll
    for (int u = 0; u < IMG_UNROLL; u++) {
      const int64_t k = k0 + u * WAVE;
      bool need = k < r.e;
      if constexpr (!ALL) {
        ci[u] = chunk_pick<OFF>(r, k, rc);
        need = need && (ci[u] & FRAME_FACES) != 0u;
      }
      j[u] = need ? list[k] : -1;
    }
#pragma unroll
    for (int u = 0; u < IMG_UNROLL; u++) {
      cj[u] = FRAME_NONE;
      if ((uint32_t)j[u] < (uint32_t)n) cj[u] = code[j[u]];  // (an entry of a failed build may be anything)
    }
#pragma unroll
    for (int u = 0; u < IMG_UNROLL; u++) {
      const int64_t k = k0 + u * WAVE;
      if constexpr (ALL) ci[u] = chunk_pick<OFF>(r, k, rc);
      if (k < r.e) images[k] = image_word(ci[u], cj[u]);
    }
  }
}

// images[k] of every entry k of the list
template <typename OFF>
__global__ void __launch_bounds__(STAGE_THREADS) k_pair_images(const OFF* __restrict__ kp, const int32_t* __restrict__ list, int32_t n_rows,
                                                            int32_t n, int64_t capacity, const uint16_t* __restrict__ code,
                                                            uint32_t* __restrict__ images, uint32_t* __restrict__ words,
                                                            const uint32_t* __restrict__ gate) {
  if (gate_closed(gate)) return;  // (nl_update_list: no build this time)
  const int lane = threadIdx.x & 63;
  const int32_t chunks = (n_rows + STAGE_ROWS - 1) / STAGE_ROWS, waves = gridDim.x * (STAGE_THREADS / WAVE);
  const bool wrapped = words[IMG_WRAPPED] != 0u;  // (uniform; no block resets it before every block has read it)
  for (int32_t c = blockIdx.x * (STAGE_THREADS / WAVE) + (threadIdx.x >> 6); c < chunks; c += waves) {
    const int32_t r0 = c * STAGE_ROWS;
    RowChunk r;
    row_chunk<OFF>(kp, n_rows, capacity, r0, lane, r);
    const uint32_t mine = lane < r.nr ? code[r0 + lane] : FRAME_NONE;
    uint32_t rc[STAGE_ROWS];  // (uniform) the codes of the chunk's rows
#pragma unroll
    for (int t = 0; t < STAGE_ROWS; t++) rc[t] = (uint32_t)__builtin_amdgcn_readlane((int32_t)mine, t);
    uint32_t any = rc[0];
#pragma unroll
    for (int t = 1; t < STAGE_ROWS; t++) any |= rc[t];
    if (!wrapped && (any & FRAME_FACES) == 0u) {  // (uniform) no row of the chunk touches a periodic face: nothing to read
      for (int64_t k = r.b + lane; k < r.e; k += WAVE) images[k] = 0u;
      continue;
    }
    if (wrapped) image_chunk<OFF, true>(r, rc, lane, list, n, code, images);
    else image_chunk<OFF, false>(r, rc, lane, list, n, code, images);
  }
  // the last block through leaves the two words at zero for the next build
  __shared__ int32_t last_s;
  __syncthreads();
  if (threadIdx.x == 0) last_s = atomicAdd(words + IMG_TICKET, 1u) == gridDim.x - 1;
  __syncthreads();
  if (last_s && threadIdx.x == 0) {
    __hip_atomic_store(words + IMG_WRAPPED, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(words + IMG_TICKET, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The open box: every image is 0.  Clears the entries of the list, [0, key_pointer[n_rows]) within the capacity.
template <typename OFF>
__global__ void __launch_bounds__(256) k_zero_images(const OFF* __restrict__ kp, int32_t n_rows, int64_t capacity,
                                                    uint32_t* __restrict__ images, const uint32_t* __restrict__ gate) {
  if (gate_closed(gate)) return;  // (nl_update_list: no build this time)
  const int64_t end = max((int64_t)0, min((int64_t)kp[n_rows], capacity));
  const int64_t quads = end >> 2;  // (the buffer is a device allocation: 16-byte aligned)
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < quads; k += (int64_t)gridDim.x * blockDim.x)
    reinterpret_cast<uint4*>(images)[k] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < end - 4 * quads) images[4 * quads + threadIdx.x] = 0u;
}

// (declared at the top of nl_api.hip) The image stage of the handle's build (h->args, h->plan), on stream s.
int launch_images(nl_handle_t h, int32_t n_rows, hipStream_t s) {
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const int32_t n = h->args.n;
    const OFF* kp = static_cast<const OFF*>(h->key_pointer);
    if (h->plan.pbc == 0) {
      const int64_t quads = std::max<int64_t>(1, h->capacity / 4);
      const dim3 grid((uint32_t)std::min<int64_t>((quads + 1023) / 1024, 8 * h->num_cus));
      hipLaunchKernelGGL(k_zero_images<OFF>, grid, dim3(256), 0, s, kp, n_rows, h->capacity, h->images, h->gate);
    } else if (n > 0 && n_rows > 0) {
      const Grid<T> g = make_grid<T>(h, h->args, h->plan.pbc);
      const int32_t cgrid = std::max(1, std::min((n + STAGE_THREADS - 1) / STAGE_THREADS, 8 * h->num_cus));
      hipLaunchKernelGGL(k_image_codes<T>, dim3(cgrid), dim3(STAGE_THREADS), 0, s, g, static_cast<const T*>(h->args.q), h->args.stride, n,
                         h->img_code, h->img_words);
      hipLaunchKernelGGL(k_pair_images<OFF>, dim3(stage_grid(h, (n_rows + STAGE_ROWS - 1) / STAGE_ROWS)), dim3(STAGE_THREADS), 0, s, kp, h->list,
                         n_rows, n, h->capacity, h->img_code, h->images, h->img_words, h->gate);
    }
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

// ------------------------------------------------------------------------------------------------- the consumer
// out[k] = {dx, dy, dz, r2} of entry k (row i, partner j, image s): S(s) in double in lattice_table's order, each component
// rounded to T once, d = (q_j + S) - q_i with one rounding per operation (components where S is 0 untouched),
// r2 = (dx^2 + dy^2) + dz^2 without FMA.  status (nl_pair_vectors_enqueue): a list whose build failed gives NaN.
template <typename T, typename OFF>
__global__ void __launch_bounds__(STAGE_THREADS) k_pair_vectors(const T* __restrict__ q, int32_t stride, const OFF* __restrict__ kp,
                                                             const int32_t* __restrict__ list, const uint32_t* __restrict__ images,
                                                             int32_t n_rows, int32_t n, int64_t capacity, T* __restrict__ out, Box box,
                                                             const uint32_t* __restrict__ status) {
  const bool failed = status && *status != 0u;  // (uniform)
  const int lane = threadIdx.x & 63;
  const int32_t chunks = (n_rows + STAGE_ROWS - 1) / STAGE_ROWS, waves = gridDim.x * (STAGE_THREADS / WAVE);
  for (int32_t c = blockIdx.x * (STAGE_THREADS / WAVE) + (threadIdx.x >> 6); c < chunks; c += waves) {
    const int32_t r0 = c * STAGE_ROWS;
    RowChunk r;
    row_chunk<OFF>(kp, n_rows, capacity, r0, lane, r);
    T xr = (T)0, yr = (T)0, zr = (T)0;  // lane t: the position of row r0 + t
    if (lane < r.nr) load_xyz(q, stride, r0 + lane, xr, yr, zr);
    for (int64_t k = r.b + lane; k - lane < r.e; k += WAVE) {
      const bool valid = k < r.e;
      const int32_t lr = chunk_row<OFF>(r, k);
      const T xi = shfl_t(xr, lr), yi = shfl_t(yr, lr), zi = shfl_t(zr, lr);  // (every lane: bpermute)
      if (!valid) continue;
      T d[4];
      if (failed) {
        d[0] = d[1] = d[2] = d[3] = (T)NAN;
      } else {
        int32_t j = list[k];
        if ((uint32_t)j >= (uint32_t)n) j = 0;
        const uint32_t w = images[k];
        T xj, yj, zj;
        load_xyz(q, stride, j, xj, yj, zj);
        if (w != 0u) {
          const double sa = (double)(int8_t)(w & 0xFFu), sb = (double)(int8_t)((w >> 8) & 0xFFu), sc = (double)(int8_t)((w >> 16) & 0xFFu);
          const double Sx = __dadd_rn(__dadd_rn(__dmul_rn(sa, box.L[0]), __dmul_rn(sb, box.xy)), __dmul_rn(sc, box.xz));
          const double Sy = __dadd_rn(__dmul_rn(sb, box.L[1]), __dmul_rn(sc, box.yz));
          const double Sz = __dmul_rn(sc, box.L[2]);
          if (Sx != 0.0) xj = add_rn(xj, (T)Sx);
          if (Sy != 0.0) yj = add_rn(yj, (T)Sy);
          if (Sz != 0.0) zj = add_rn(zj, (T)Sz);
        }
        d[0] = sub_rn(xj, xi), d[1] = sub_rn(yj, yi), d[2] = sub_rn(zj, zi);
        d[3] = add_rn(add_rn(mul_rn(d[0], d[0]), mul_rn(d[1], d[1])), mul_rn(d[2], d[2]));
      }
      T* o = out + (size_t)k * 4;
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(o) = make_float4(d[0], d[1], d[2], d[3]);
      } else {
        reinterpret_cast<double2*>(o)[0] = make_double2(d[0], d[1]);
        reinterpret_cast<double2*>(o)[1] = make_double2(d[2], d[3]);
      }
    }
  }
}

int pair_vectors_launch(nl_handle_t h, const void* q_dev, int32_t stride, void* out_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n_rows = h->n_rows;
  if (n_rows <= 0) return NL_OK;
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    hipLaunchKernelGGL((k_pair_vectors<T, OFF>), dim3(stage_grid(h, (n_rows + STAGE_ROWS - 1) / STAGE_ROWS)), dim3(STAGE_THREADS), 0, s,
                       static_cast<const T*>(q_dev), stride, static_cast<const OFF*>(h->key_pointer), h->list, h->images, n_rows, h->n,
                       h->capacity, static_cast<T*>(out_dev), h->plan.box, status);  // (the build's box, as k_lj)
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

// nl_pair_vectors; enqueue: without the wait, stream-ordered behind the update (or completed build) whose list it reads.
int pair_vectors_call(nl_handle_t h, const void* q_dev, int32_t q_stride, void* out_dev, hipStream_t s, bool enqueue) {
  if (!h || !q_dev || !out_dev || (q_stride != 3 && q_stride != 4)) return fail(h, NL_ERR_ARG);
  if (!h->pair_images) return fail(h, NL_ERR_STATE);
  if (int rc = consumer_ready(h, s, enqueue)) return rc;
  if (!h->plan.images) return fail(h, NL_ERR_STATE);
  HIPCHK(h, hipSetDevice(h->device));
  return pair_vectors_launch(h, q_dev, q_stride, out_dev, s, enqueue ? h->status : nullptr);
}

}  // namespace

extern "C" {

int nl_set_pair_images(nl_handle_t h, int on) {
  if (!h) return NL_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) (void)finish(h, false);
  if ((on != 0) == h->pair_images) return NL_OK;  // (the same value again changes nothing)
  h->upd_valid = false;
  if (on) {
    h->pair_images = true;
    if (int rc = images_reserve(h)) {  // no room for the images: the flag stays off
      images_release(h);
      h->pair_images = false;
      return rc;
    }
  } else {
    HIPCHK(h, hipDeviceSynchronize());  // (replays of a graph the caller captured may still write the images)
    images_release(h);
    h->pair_images = false;
  }
  h->built = false;
  h->t_valid = false;
  return NL_OK;
}

int nl_get_pair_images(nl_handle_t h, const int8_t** images_dev, int64_t* nentries) {
  if (!h) return NL_ERR_ARG;
  if (!h->pair_images) return fail(h, NL_ERR_STATE);
  int rc = nl_synchronize(h);
  if (rc) return rc;
  if (!h->plan.images) return fail(h, NL_ERR_STATE);
  if (images_dev) *images_dev = reinterpret_cast<const int8_t*>(h->images.get());
  if (nentries) *nentries = list_total(h);
  return NL_OK;
}

int nl_pair_vectors(nl_handle_t h, const void* q_dev, int32_t q_stride, void* out_dev, void* stream) {
  return pair_vectors_call(h, q_dev, q_stride, out_dev, (hipStream_t)stream, false);
}
int nl_pair_vectors_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* out_dev, void* stream) {
  return pair_vectors_call(h, q_dev, q_stride, out_dev, (hipStream_t)stream, true);
}

}  // extern "C"
