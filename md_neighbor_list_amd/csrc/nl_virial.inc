// nl_virial.inc -- the totals of the Lennard-Jones consumer (DESIGN.md sections 8k, 8l): the virial tensor W_ab = sum d_a F_b,
// the potential energy U and the number of pairs within rc_force, over the entries of the last build's list.  The pair's
// values come from the walk that gives nl_lj_forces its pairs (lj_row_pairs of nl_consumer.inc: lj_image + lj_pair), so
// the totals belong to those forces; the rule is stated at nl_lj_virial in include/nl_hip.h.  The launch arguments
// (lj_args) and the entry points' checks (lj_call over consumer_call) are the forces' too; the launch of the totals
// (totals_launch) and the tree over a block (block_tree) are written here for every pair function (DESIGN.md section 8q).  No entry scatters anything (a stored pair
// contributes once, in the row that stores it), so the half list needs no atomics, and nothing here is a floating-point
// atomic: every sum has one fixed order,
//   lane: its entries, row after row      wave: the butterfly of wave_sum      block: waves 0, 1, 2, 3
//   k_virial_reduce: thread t the partials t, t + 256, ...; then block_tree over the 256 threads
// and two calls on the same list and positions give the same 64 bytes.
// Included at the end of nl_api.hip, behind nl_consumer.inc.

namespace {

constexpr int VIR_BLOCKS = NL_VIRIAL_BLOCKS;  // the most blocks of k_lj_virial, and the rows of vir_part
constexpr int VIR_OUT = 8;                    // W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in
static_assert(VIR_BLOCKS <= 2048 && STAGE_THREADS == 4 * WAVE, "vir_part holds a 64-byte partial per block of 4 waves");

// One wave per row (lj_row_pairs of nl_consumer.inc), the rows dealt to the waves of the grid in turn; every lane keeps its
// 8 sums in double across all its rows.  A term is computed in T (one rounding each: the build has no contraction) and
// converted, which is exact.
// ghost_w: the weight of an entry whose partner is a ghost (LjPartner of nl_consumer.inc; a local-id slab build), against 1 for
// every other entry: 1/2 after a half build, where the partner's owner stores the pair too, 1 after a full one, whose every
// entry is halved by k_virial_reduce.  The weight goes into the sum's fma: w t is exact (a power of two), so fma(1, t, acc) is
// acc + t, bit for bit what a whole build has always summed.
// A failed list (status, the enqueue variants) is not read: the partials are zero and k_virial_reduce writes the NaN.
template <typename T, typename OFF, bool TRI, typename PAR>
__device__ __forceinline__ void lj_virial_rows(const LjArgs<T, OFF>& a, const PAR& p, double ghost_w, double* __restrict__ part) {
  __shared__ double red[4][VIR_OUT];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[VIR_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool live = !(a.status && *a.status != 0u);  // (uniform over the launch)
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; live && row < a.n; row += (int32_t)gridDim.x * 4) {
    lj_row_pairs<T, OFF, TRI>(a, p, row, lane, [&](int32_t, LjPartner w, T dx, T dy, T dz, T fx, T fy, T fz, T pe, bool in) {
      const T wxx = fx * dx, wyy = fy * dy, wzz = fz * dz, wxy = fx * dy, wxz = fx * dz, wyz = fy * dz;
      const double c = w.ghost ? ghost_w : 1.0;
      acc[0] = fma(c, (double)wxx, acc[0]), acc[1] = fma(c, (double)wyy, acc[1]), acc[2] = fma(c, (double)wzz, acc[2]);
      acc[3] = fma(c, (double)wxy, acc[3]), acc[4] = fma(c, (double)wxz, acc[4]), acc[5] = fma(c, (double)wyz, acc[5]);
      acc[6] = fma(c, (double)pe, acc[6]);  // (+-0 outside rc_force, as the forces)
      acc[7] += in ? c : 0.0;
      if constexpr (PAR::table) acc[7] += (in && pe != pe) ? (double)NAN : 0.0;  // (a pair below the table: all 8 are NaN)
    });
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

template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_lj_virial(LjArgs<T, OFF> a, LjScalars<T> p, double ghost_w, double* __restrict__ part) {
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}
template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_lj_virial_typed(LjArgs<T, OFF> a, LjByType<T> p, double ghost_w, double* __restrict__ part) {
  lj_virial_rows<T, OFF, TRI>(a, p, ghost_w, part);
}

// The sum of a block in one fixed order (k_virial_reduce, k_eam_fe_part): every thread brings the C sums of
// its own strided walk, then a tree over the threads; the block's sums are sm[c][0] of what it returns.
template <int C> __device__ __forceinline__ auto& block_tree(const double (&s)[C]) {
  __shared__ double sm[C][STAGE_THREADS];
  const int32_t t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < C; c++) sm[c][t] = s[c];
  __syncthreads();
  for (int32_t d = STAGE_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
#pragma unroll
      for (int c = 0; c < C; c++) sm[c][t] += sm[c][t + d];
    }
    __syncthreads();
  }
  return sm;
}

// One block: thread t adds the partials t, t + 256, ... in that order, then block_tree.  scale: 1 after a half build, 1/2
// after a full one, whose list holds every pair twice (exact).  A failed list gives 8 NaN.
__global__ void __launch_bounds__(STAGE_THREADS) k_virial_reduce(const double* __restrict__ part, int32_t nblk, double scale,
                                                                 double* __restrict__ out, const uint32_t* __restrict__ status) {
  const int32_t t = threadIdx.x;
  double s[VIR_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int32_t b = t; b < nblk; b += STAGE_THREADS) {
#pragma unroll
    for (int c = 0; c < VIR_OUT; c++) s[c] += part[(size_t)b * VIR_OUT + c];
  }
  const auto& sm = block_tree(s);
  if (t < VIR_OUT) out[t] = (status && *status != 0u) ? (double)NAN : scale * sm[t][0];
}

// A launch of the 8 totals into out_dev (the Lennard-Jones, table and EAM totals): zeroes for an empty list; vir_part; the
// arguments; body(Inst, LjArgs, nblk, part) launches the family's kernel on nblk <= max_blocks blocks, which leave their
// partials in part, and returns a status; k_virial_reduce.
template <typename BODY>
int totals_launch(nl_handle_t h, const void* q_dev, int32_t stride, double* out_dev, hipStream_t s, const uint32_t* status, int32_t max_blocks,
                  BODY&& body) {
  const int32_t n = h->n_rows;
  if (n == 0) {
    HIPCHK(h, hipMemsetAsync(out_dev, 0, sizeof(double) * VIR_OUT, s));
    return NL_OK;
  }
  if (int rc = first_call_scratch(h, h->vir_part, sizeof(double) * VIR_OUT * VIR_BLOCKS, s)) return rc;
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, max_blocks);
  double* part = h->vir_part;
  const int rc = dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    int rb = NL_OK;
    with_flag(h->plan.tilt, [&](auto tri) { rb = body(Inst<T, OFF, false, decltype(tri)::value>(), a, nblk, part); });
    if (rb) return rb;
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_virial_reduce, dim3(1), dim3(STAGE_THREADS), 0, s, part, nblk, h->plan.full ? 0.5 : 1.0, out_dev, status);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

// lj: {epsilon, sigma, rc_force} of the launch; nullptr: by type, from the handle's tables (as lj_launch).
int virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, const double* lj, double* out_dev, hipStream_t s,
                  const uint32_t* status) {
  const double ghost_w = h->plan.full ? 1.0 : 0.5;
  return totals_launch(h, q_dev, stride, out_dev, s, status, VIR_BLOCKS, [&](auto i, const auto& a, int32_t nblk, double* part) {
    using I = decltype(i);
    using T = typename I::T;
    if (lj) hipLaunchKernelGGL((k_lj_virial<T, typename I::OFF, I::tri>), dim3(nblk), dim3(STAGE_THREADS), 0, s, a, lj_scalars<T>(lj), ghost_w, part);
    else hipLaunchKernelGGL((k_lj_virial_typed<T, typename I::OFF, I::tri>), dim3(nblk), dim3(STAGE_THREADS), 0, s, a, lj_by_type<T>(h), ghost_w, part);
    return NL_OK;
  });
}

}  // namespace

extern "C" {  // (the checks: lj_call of nl_consumer.inc)

int nl_lj_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force, double* out_dev,
                 void* stream) {
  const double lj[3] = {epsilon, sigma, rc_force};
  return lj_call(h, q_dev, q_stride, lj, out_dev, stream, false, virial_launch);
}
int nl_lj_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force,
                         double* out_dev, void* stream) {
  const double lj[3] = {epsilon, sigma, rc_force};
  return lj_call(h, q_dev, q_stride, lj, out_dev, stream, true, virial_launch);
}
int nl_lj_virial_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return lj_call(h, q_dev, q_stride, nullptr, out_dev, stream, false, virial_launch);
}
int nl_lj_virial_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  return lj_call(h, q_dev, q_stride, nullptr, out_dev, stream, true, virial_launch);
}

}  // extern "C"
