// nl_transpose.inc -- the GPU class's output format (neighlist_gpu.hpp:468-482): the FULL list (both directions) in
// the transposed layout list[k*N + i].  Included at the end of nl_api.hip.
//  * after a NL_LIST_FULL build: the full CSR is converted in one pass with coalesced writes (k_csr_to_transposed);
//  * after a NL_LIST_HALF build: derived from the half list: row i keeps its own partners (j > i) in rows
//    k < half[i], and every pair (i,j) also lands in column j at row half[j] + (arrival order) -- scattered.
// The order inside a column is free (the reference's check sorts it, make_list.cu:178-185).

namespace {

__global__ void __launch_bounds__(256) k_full_init(const int32_t* __restrict__ half, int32_t n,
                                                    int32_t* __restrict__ full, int32_t* __restrict__ cursor) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) full[i] = half[i], cursor[i] = 0;
}

// one wave per row: full[j] += 1 for every partner j
__global__ void __launch_bounds__(256) k_full_count(const int32_t* __restrict__ kp, const int32_t* __restrict__ list,
                                                     int32_t n, int32_t* __restrict__ full) {
  const int32_t row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= n) return;
  for (int32_t e = kp[row] + lane; e < kp[row + 1]; e += 64) atomicAdd(&full[list[e]], 1);
}

__global__ void __launch_bounds__(256) k_max(const int32_t* __restrict__ v, int32_t n, int32_t* __restrict__ out) {
  __shared__ int32_t wmax[4];
  int32_t m = 0;
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) m = max(m, v[i]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_xor(m, d, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));  // one atomic per block
}

__global__ void __launch_bounds__(256) k_transpose(const int32_t* __restrict__ kp, const int32_t* __restrict__ list,
                                                    const int32_t* __restrict__ half, int32_t n, int64_t stride,
                                                    int32_t* __restrict__ t, int32_t* __restrict__ cursor) {
  const int32_t row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= n) return;
  const int32_t b = kp[row], e = kp[row + 1];
  for (int32_t k = lane; k < e - b; k += 64) {
    const int32_t j = list[b + k];
    t[(int64_t)k * stride + row] = j;
    const int32_t slot = half[j] + atomicAdd(&cursor[j], 1);
    t[(int64_t)slot * stride + j] = row;
  }
}

// Full CSR (NL_LIST_FULL build) -> list[k*N + i], 64 consecutive rows per workgroup.  The rows of a block are ONE
// contiguous piece of the CSR (~37 KB at cfg 2): it is copied into LDS as it lies (LDS-DMA, every load aligned and in
// flight together), then every wave writes k-rows: lane l reads entry k of row i0 + l from the flat copy and the 64
// lanes store 256 consecutive bytes.  Blocks whose rows exceed the LDS piece take the tiled kernel below.
constexpr int TR_FLAT_WORDS = 12288;  // 48 KB: 3 workgroups per CU
__global__ void __launch_bounds__(256) k_csr_to_transposed_flat(const int32_t* __restrict__ kp, const int32_t* __restrict__ list,
                                                                int32_t n, int64_t stride, int32_t* __restrict__ t,
                                                                int32_t* __restrict__ big_blocks) {
  __shared__ __attribute__((aligned(32))) int32_t flat[TR_FLAT_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int32_t i0 = blockIdx.x * 64, i1 = min(i0 + 64, n);
  const int32_t b0 = kp[i0], len = kp[i1] - b0;
  if (len > TR_FLAT_WORDS) {  // (uniform) left to the tiled kernel
    if (tid == 0) big_blocks[atomicAdd(big_blocks - 1, 1)] = blockIdx.x;
    return;
  }
  const int32_t i = min(i0 + lane, n - 1);
  const int32_t my_beg = kp[i] - b0, my_cnt = i0 + lane < n ? kp[i + 1] - kp[i] : 0;
  for (int32_t p0 = wave * 64; p0 < len; p0 += 256) {
    if (p0 + lane < len)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(list + b0 + p0 + lane),
                                       (__attribute__((address_space(3))) void*)(flat + p0), 4, 0, 0);
  }
  int32_t mx = my_cnt;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
  __syncthreads();
  for (int32_t k = wave; k < mx; k += 4)
    if (k < my_cnt) t[(int64_t)k * stride + i0 + lane] = flat[my_beg + k];
}

// The same through a 64 x 64 LDS tile (rows of any length): a block owns 64 consecutive rows;
// per chunk of 64 k its waves read row by row (64 consecutive entries of one CSR row per instruction) and write
// k by k (64 consecutive rows of one k-row per instruction): both sides coalesced.
__global__ void __launch_bounds__(256) k_csr_to_transposed(const int32_t* __restrict__ kp, const int32_t* __restrict__ list,
                                                           int32_t n, int64_t stride, int32_t* __restrict__ t,
                                                           const int32_t* __restrict__ big_blocks) {
  __shared__ int32_t tile[64][65];  // +1: the k-by-k reads walk a column
  __shared__ int32_t s_beg[64], s_cnt[64], s_max;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // big_blocks: the 64-row blocks the flat kernel left (count at big_blocks[-1]); NULL = every block
  if (big_blocks && (int32_t)blockIdx.x >= big_blocks[-1]) return;
  const int32_t i0 = (big_blocks ? big_blocks[blockIdx.x] : (int32_t)blockIdx.x) * 64;
  if (tid < 64) {
    const int32_t i = i0 + tid;
    int32_t b = 0, cnt = 0;
    if (i < n) b = kp[i], cnt = kp[i + 1] - b;
    s_beg[tid] = b, s_cnt[tid] = cnt;
    int32_t mx = cnt;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    if (tid == 0) s_max = mx;
  }
  __syncthreads();
  const int32_t mx = s_max, my_cnt = s_cnt[lane];
  for (int32_t k0 = 0; k0 < mx; k0 += 64) {
    // read: row r, entries k0 + lane -- the wave's 16 rows loaded before the first LDS write (unconditional loads of a
    // valid entry, kept in flight together: as a loop of "if (k < cnt) tile = list[..]" every load was waited for before
    // the next was issued, 48 dependent round trips per block)
    int32_t v[16];
    const int32_t k = k0 + lane;
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int r = wave + 4 * u;
      v[u] = list[k < s_cnt[r] ? s_beg[r] + k : 0];
    }
#pragma unroll
    for (int u = 0; u < 16; u++) asm volatile("" : "+v"(v[u]));
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int r = wave + 4 * u;
      if (k < s_cnt[r]) tile[r][lane] = v[u];
    }
    __syncthreads();
    for (int kk = wave; kk < 64; kk += 4) {  // write: k-row k0 + kk, rows i0 + lane
      const int32_t k = k0 + kk;
      if (k < my_cnt) t[(int64_t)k * stride + i0 + lane] = tile[lane][kk];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int nl_get_full_transposed(nl_handle_t h, const int32_t** list_dev, const int32_t** count_dev,
                                      int64_t* row_stride, int32_t* max_partners) {
  if (!h) return NL_ERR_ARG;
  int rc = nl_synchronize(h);
  if (rc) return rc;
  if (h->args.slab || h->n_rows != h->n) return fail(h, NL_ERR_STATE);  // ids must be row indices
  const int32_t n = h->n;
  // this layout is the reference GPU class's (int32 throughout, neighlist_gpu.hpp:468-487): a list that an int32
  // key_pointer cannot address has no transposed form
  const void* kp_any = nullptr;
  if (!h->t_valid && (rc = key_pointer_as(h, 32, &kp_any))) return rc;
  const int32_t* const kp32 = static_cast<const int32_t*>(kp_any);
  if (!h->t_valid && h->plan.full) {
    // the build produced the full CSR: counts are the full counts already, one coalesced conversion pass
    hipStream_t s = h->own_stream;
    HIPCHK(h, hipStreamSynchronize(h->last_stream));
    const int32_t nb = (n + 255) / 256;
    int32_t mx = 0;
    if (n > 0) {
      HIPCHK(h, hipMemsetAsync(h->totals + 2, 0, 8, s));
      hipLaunchKernelGGL(k_max, dim3(std::min(nb, 1024)), dim3(256), 0, s, h->count, n,
                         reinterpret_cast<int32_t*>(h->totals + 2));
      HIPCHK(h, hipMemcpyAsync(&mx, h->totals + 2, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
    }
    // rows: the reference allocates MAX_PARTNERS = 200 (neighlist_gpu.hpp:72); keep at least that many so that the
    // buffer is not reallocated (and refilled with -1) whenever the longest row grows by one
    const int64_t rows = std::max<int32_t>(mx, 200);
    if (rows * (int64_t)std::max(n, 1) > h->t_rows_cap) {
      if ((rc = dev_alloc(h, h->t_list, 4 * (size_t)(rows * std::max(n, 1))))) return rc;
      h->t_rows_cap = rows * std::max(n, 1);
      HIPCHK(h, hipMemsetAsync(h->t_list, 0xFF, 4 * (size_t)h->t_rows_cap, s));  // -1 fill, once (neighlist_gpu.hpp:271)
    }
    if (n > 0) {
      // flat kernel first; the blocks whose 64 rows exceed its LDS piece are listed (in t_cursor, unused after a full
      // build) and done by the tiled kernel, whose other workgroups leave at once
      const int32_t nblk = (n + 63) / 64;
      // (one int per particle of n_max, as the half path sizes it: nblk + 1 <= n_max + 16; nl_initialize releases it)
      if ((rc = follow(h, h->t_cursor, h->n_max, 4 * ((size_t)h->n_max + 16)))) return rc;
      int32_t* const big = h->t_cursor + 1;  // [-1] = count
      HIPCHK(h, hipMemsetAsync(h->t_cursor, 0, 4, s));
      hipLaunchKernelGGL(k_csr_to_transposed_flat, dim3(nblk), dim3(256), 0, s, kp32, h->list, n, (int64_t)n, h->t_list, big);
      hipLaunchKernelGGL(k_csr_to_transposed, dim3(nblk), dim3(256), 0, s, kp32, h->list, n, (int64_t)n, h->t_list,
                         static_cast<const int32_t*>(big));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    h->t_max = mx;
    h->t_valid = true;
  }
  if (!h->t_valid) {
    hipStream_t s = h->own_stream;
    HIPCHK(h, hipStreamSynchronize(h->last_stream));
    // one count and one cursor per particle of the handle's n_max (nl_initialize releases both: a handle that has grown
    // since the last fetch gets them anew)
    if ((rc = follow(h, h->t_count, h->n_max, 4 * ((size_t)h->n_max + 16)))) return rc;
    if ((rc = follow(h, h->t_cursor, h->n_max, 4 * ((size_t)h->n_max + 16)))) return rc;
    const int32_t nb = (n + 255) / 256, nbw = (int32_t)(((int64_t)n * 64 + 255) / 256);
    int32_t mx = 0;
    if (n > 0) {
      hipLaunchKernelGGL(k_full_init, dim3(nb), dim3(256), 0, s, h->count, n, h->t_count, h->t_cursor);
      hipLaunchKernelGGL(k_full_count, dim3(nbw), dim3(256), 0, s, kp32, h->list, n, h->t_count);
      HIPCHK(h, hipMemsetAsync(h->totals + 2, 0, 8, s));
      hipLaunchKernelGGL(k_max, dim3(std::min(nb, 1024)), dim3(256), 0, s, h->t_count, n,
                         reinterpret_cast<int32_t*>(h->totals + 2));
      HIPCHK(h, hipMemcpyAsync(&mx, h->totals + 2, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
    }
    const int64_t rows = std::max<int32_t>(mx, 1);
    if (rows * (int64_t)std::max(n, 1) > h->t_rows_cap) {
      if ((rc = dev_alloc(h, h->t_list, 4 * (size_t)(rows * std::max(n, 1))))) return rc;
      h->t_rows_cap = rows * std::max(n, 1);
    }
    if (n > 0) {
      HIPCHK(h, hipMemsetAsync(h->t_list, 0xFF, 4 * (size_t)(rows * n), s));  // -1 fill, neighlist_gpu.hpp:271
      hipLaunchKernelGGL(k_transpose, dim3(nbw), dim3(256), 0, s, kp32, h->list, h->count, n, (int64_t)n,
                         h->t_list, h->t_cursor);
      HIPCHK(h, hipStreamSynchronize(s));
    }
    HIPCHK(h, hipGetLastError());
    h->t_max = mx;
    h->t_valid = true;
  }
  if (list_dev) *list_dev = h->t_list;
  if (count_dev) *count_dev = h->plan.full ? h->count : h->t_count;
  if (row_stride) *row_stride = n;
  if (max_partners) *max_partners = h->t_max;
  return NL_OK;
}
