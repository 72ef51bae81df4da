// nl_virial.inc -- the totals of the Lennard-Jones consumer (DESIGN.md section 8k): the virial tensor W_ab = sum d_a F_b,
// the potential energy U and the number of pairs within rc_force, over the entries of the last build's list.  The pair
// is lj_image + lj_pair of nl_consumer.inc, so the totals belong to the forces nl_lj_forces returns; the rule is stated at
// nl_lj_virial in include/nl_hip.h.  No entry scatters anything (a stored pair contributes once, in the row that stores
// it), so the half list needs no atomics, and nothing here is a floating-point atomic: every sum has one fixed order,
//   lane: its entries, row after row      wave: the butterfly of wave_sum      block: waves 0, 1, 2, 3
//   k_virial_reduce: thread t the partials t, t + 256, ...; then a tree over the 256 threads
// and two calls on the same list and positions give the same 64 bytes.
// Included at the end of nl_api.hip, behind nl_consumer.inc.

namespace {

constexpr int VIR_BLOCKS = NL_VIRIAL_BLOCKS;  // the most blocks of k_lj_virial, and the rows of vir_part
constexpr int VIR_OUT = 8;                    // W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in
static_assert(VIR_BLOCKS <= 2048 && STAGE_THREADS == 4 * WAVE, "vir_part holds a 64-byte partial per block of 4 waves");

// One wave per row, the rows dealt to the waves of the grid in turn; every lane keeps its 8 sums in double across all its
// rows.  A term is computed in T (one rounding each: the build has no contraction) and converted, which is exact.
// By type: as lj_row, lane t < ntypes holds the parameters of (t_row, t) and every lane stays in the loop for the pick.
// A failed list (status, the enqueue variants) is not read: the partials are zero and k_virial_reduce writes the NaN.
template <typename T, typename OFF, bool TRI, typename PAR>
__device__ __forceinline__ void lj_virial_rows(const T* __restrict__ q, int32_t stride, const OFF* __restrict__ kp,
                                               const int32_t* __restrict__ list, int32_t n, const PAR& p, double* __restrict__ part,
                                               T Lx, T Ly, T Lz, const uint32_t* __restrict__ status, T xy, T xz, T yz) {
  __shared__ double red[4][VIR_OUT];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[VIR_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool live = !(status && *status != 0u);  // (uniform over the launch)
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; live && row < n; row += (int32_t)gridDim.x * 4) {
    T eps4, sig2, rcf2;
    if constexpr (PAR::typed) {
      constexpr int NT2 = NL_MAX_TYPES * NL_MAX_TYPES;
      const int32_t at = (p.types[row] & (NL_MAX_TYPES - 1)) * NL_MAX_TYPES + (lane & (NL_MAX_TYPES - 1));
      eps4 = p.par[at], sig2 = p.par[NT2 + at], rcf2 = p.par[2 * NT2 + at];
    } else {
      eps4 = p.eps4, sig2 = p.sig2, rcf2 = p.rcf2;
    }
    T xi, yi, zi;
    load_xyz(q, stride, row, xi, yi, zi);
    const OFF b = kp[row], e = kp[row + 1];
    for (OFF k = b + lane; (PAR::typed ? k - lane : k) < e; k += 64) {
      const bool valid = !PAR::typed || k < e;
      const int32_t j = valid ? list[k] : row;
      T e4 = eps4, s2 = sig2, c2 = rcf2;
      if constexpr (PAR::typed) {
        const int32_t tj = p.types[j] & (NL_MAX_TYPES - 1);
        e4 = shfl_t(eps4, tj), s2 = shfl_t(sig2, tj), c2 = shfl_t(rcf2, tj);
        if (!valid) continue;
      }
      T xj, yj, zj;
      load_xyz(q, stride, j, xj, yj, zj);
      T dx, dy, dz, fx, fy, fz, pe;
      bool in;
      lj_image<T, TRI>(xi, yi, zi, xj, yj, zj, dx, dy, dz, Lx, Ly, Lz, xy, xz, yz);
      lj_pair<T>(dx, dy, dz, e4, s2, c2, fx, fy, fz, pe, in);
      const T wxx = fx * dx, wyy = fy * dy, wzz = fz * dz, wxy = fx * dy, wxz = fx * dz, wyz = fy * dz;
      acc[0] += (double)wxx, acc[1] += (double)wyy, acc[2] += (double)wzz;
      acc[3] += (double)wxy, acc[4] += (double)wxz, acc[5] += (double)wyz;
      acc[6] += (double)pe;  // (+-0 outside rc_force, as the forces)
      acc[7] += in ? 1.0 : 0.0;
    }
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
__global__ void __launch_bounds__(STAGE_THREADS) k_lj_virial(const T* __restrict__ q, int32_t stride, const OFF* __restrict__ kp,
                                                             const int32_t* __restrict__ list, int32_t n, T eps4, T sig2, T rcf2,
                                                             double* __restrict__ part, T Lx, T Ly, T Lz,
                                                             const uint32_t* __restrict__ status, T xy, T xz, T yz) {
  lj_virial_rows<T, OFF, TRI>(q, stride, kp, list, n, LjScalars<T>{eps4, sig2, rcf2}, part, Lx, Ly, Lz, status, xy, xz, yz);
}
template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_lj_virial_typed(const T* __restrict__ q, int32_t stride, const OFF* __restrict__ kp,
                                                                   const int32_t* __restrict__ list, int32_t n,
                                                                   const int32_t* __restrict__ types, const T* __restrict__ par,
                                                                   double* __restrict__ part, T Lx, T Ly, T Lz,
                                                                   const uint32_t* __restrict__ status, T xy, T xz, T yz) {
  lj_virial_rows<T, OFF, TRI>(q, stride, kp, list, n, LjByType<T>{types, par}, part, Lx, Ly, Lz, status, xy, xz, yz);
}

// One block: thread t adds the partials t, t + 256, ... in that order, then a tree over the threads.  scale: 1 after a
// half build, 1/2 after a full one, whose list holds every pair twice (exact).  A failed list gives 8 NaN.
__global__ void __launch_bounds__(STAGE_THREADS) k_virial_reduce(const double* __restrict__ part, int32_t nblk, double scale,
                                                                 double* __restrict__ out, const uint32_t* __restrict__ status) {
  __shared__ double sm[VIR_OUT][STAGE_THREADS];
  const int32_t t = threadIdx.x;
  double s[VIR_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int32_t b = t; b < nblk; b += STAGE_THREADS) {
#pragma unroll
    for (int c = 0; c < VIR_OUT; c++) s[c] += part[(size_t)b * VIR_OUT + c];
  }
#pragma unroll
  for (int c = 0; c < VIR_OUT; c++) sm[c][t] = s[c];
  __syncthreads();
  for (int32_t d = STAGE_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
#pragma unroll
      for (int c = 0; c < VIR_OUT; c++) sm[c][t] += sm[c][t + d];
    }
    __syncthreads();
  }
  if (t < VIR_OUT) out[t] = (status && *status != 0u) ? (double)NAN : scale * sm[t][0];
}

// lj: {epsilon, sigma, rc_force} of the launch; nullptr: by type, from the handle's tables (as lj_launch).
int virial_launch(nl_handle_t h, const void* q_dev, int32_t stride, const double* lj, double* out_dev, hipStream_t s,
                  const uint32_t* status) {
  const int32_t n = h->n;
  if (n == 0) {
    HIPCHK(h, hipMemsetAsync(out_dev, 0, sizeof(double) * VIR_OUT, s));
    return NL_OK;
  }
  if (!h->vir_part) {  // the first call: a stream that is being captured cannot allocate
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(h, hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(h, NL_ERR_STATE);
    if (int rc = side_alloc(h, h->vir_part, sizeof(double) * VIR_OUT * VIR_BLOCKS)) return rc;
  }
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, VIR_BLOCKS);
  double* part = h->vir_part;
  const int rc = dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const Box& b = h->plan.box;  // the build's box and mask, as lj_launch
    const T Lx = (h->plan.pbc & 1) ? (T)b.L[0] : (T)0, Ly = (h->plan.pbc & 2) ? (T)b.L[1] : (T)0, Lz = (h->plan.pbc & 4) ? (T)b.L[2] : (T)0;
    const T xy = (T)b.xy, xz = (T)b.xz, yz = (T)b.yz;
    const T* q = static_cast<const T*>(q_dev);
    const OFF* kp = static_cast<const OFF*>(h->key_pointer);
    auto launch = [&](auto tri) {
      constexpr bool R = decltype(tri)::value;
      if (lj)
        hipLaunchKernelGGL((k_lj_virial<T, OFF, R>), dim3(nblk), dim3(STAGE_THREADS), 0, s, q, stride, kp, h->list, n, (T)(4.0 * lj[0]),
                           (T)(lj[1] * lj[1]), (T)(lj[2] * lj[2]), part, Lx, Ly, Lz, status, xy, xz, yz);
      else
        hipLaunchKernelGGL((k_lj_virial_typed<T, OFF, R>), dim3(nblk), dim3(STAGE_THREADS), 0, s, q, stride, kp, h->list, n, h->ty_types,
                           static_cast<const T*>(h->lj_par), part, Lx, Ly, Lz, status, xy, xz, yz);
    };
    h->plan.tilt ? launch(std::true_type()) : launch(std::false_type());
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_virial_reduce, dim3(1), dim3(STAGE_THREADS), 0, s, part, nblk, h->plan.full ? 0.5 : 1.0, out_dev, status);
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

}  // namespace

extern "C" {

int nl_lj_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force, double* out_dev,
                 void* stream) {
  if (!h || !q_dev || !out_dev || (q_stride != 3 && q_stride != 4) || !(rc_force > 0) || !(sigma > 0)) return fail(h, NL_ERR_ARG);
  if (int rc = consumer_ready(h, (hipStream_t)stream, false)) return rc;
  if (rc_force > h->rc) return fail(h, NL_ERR_ARG);  // the list does not reach that far
  HIPCHK(h, hipSetDevice(h->device));
  const double lj[3] = {epsilon, sigma, rc_force};
  return virial_launch(h, q_dev, q_stride, lj, out_dev, (hipStream_t)stream, nullptr);
}

int nl_lj_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force,
                         double* out_dev, void* stream) {
  if (!h || !q_dev || !out_dev || (q_stride != 3 && q_stride != 4) || !(rc_force > 0) || !(sigma > 0)) return fail(h, NL_ERR_ARG);
  if (!(rc_force <= h->rc - h->skin)) return fail(h, NL_ERR_ARG);  // beyond what a list reused within the skin guarantees
  if (int rc = consumer_ready(h, (hipStream_t)stream, true)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const double lj[3] = {epsilon, sigma, rc_force};
  return virial_launch(h, q_dev, q_stride, lj, out_dev, (hipStream_t)stream, h->status);
}

int nl_lj_virial_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  if (!h || !q_dev || !out_dev || (q_stride != 3 && q_stride != 4)) return fail(h, NL_ERR_ARG);
  if (int rc = consumer_ready(h, (hipStream_t)stream, false)) return rc;
  if (int rc = lj_typed_check(h, 0.0)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return virial_launch(h, q_dev, q_stride, nullptr, out_dev, (hipStream_t)stream, nullptr);
}

int nl_lj_virial_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream) {
  if (!h || !q_dev || !out_dev || (q_stride != 3 && q_stride != 4)) return fail(h, NL_ERR_ARG);
  if (int rc = lj_typed_check(h, h->skin)) return rc;
  if (int rc = consumer_ready(h, (hipStream_t)stream, true)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return virial_launch(h, q_dev, q_stride, nullptr, out_dev, (hipStream_t)stream, h->status);
}

}  // extern "C"
