// nl_consumer.inc -- a consumer of the list (SURVEY.md section 8 f3): truncated Lennard-Jones forces and per-particle
// potential energy from the CSR of the last build.  Absent in the reference (it allocates a momentum array and never
// uses it, make_list.cpp:135,138-140); here it answers which list kind the builder should be optimised for.
//   full list: row i gathers its partners and writes f[i] once -- no atomics, every pair evaluated twice;
//   half list: every pair once, the reaction goes to f[j] with floating-point atomics.
// Included at the end of nl_api.hip.

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

// The image of a pair of the list's build.  Orthogonal box: one half-box test per periodic axis (L > 0; 0 = open axis).
// Triclinic box (TRI: nl_set_box with a tilt): fold z, y, x in T with rint, as the skin check does in double -- one test per
// axis is not enough there (after the z fold dy can exceed 1.5 Ly once yz is large).  Every component of the image within rc
// is below L_d / 2, so this finds the image the list used.
template <typename T> __device__ __forceinline__ T rint_t(T v) {
  if constexpr (sizeof(T) == 4) return rintf(v);
  else return rint(v);
}
template <typename T, bool TRI>
__device__ __forceinline__ void lj_image(T& dx, T& dy, T& dz, T Lx, T Ly, T Lz, T xy, T xz, T yz) {
  if constexpr (TRI) {
    if (Lz > (T)0) {
      const T k = rint_t(dz / Lz);
      dz = dz - k * Lz, dy = dy - k * yz, dx = dx - k * xz;
    }
    if (Ly > (T)0) {
      const T k = rint_t(dy / Ly);
      dy = dy - k * Ly, dx = dx - k * xy;
    }
    if (Lx > (T)0) dx = dx - rint_t(dx / Lx) * Lx;
  } else {
    if (Lx > (T)0) dx = dx > (T)0.5 * Lx ? dx - Lx : dx < (T)-0.5 * Lx ? dx + Lx : dx;
    if (Ly > (T)0) dy = dy > (T)0.5 * Ly ? dy - Ly : dy < (T)-0.5 * Ly ? dy + Ly : dy;
    if (Lz > (T)0) dz = dz > (T)0.5 * Lz ? dz - Lz : dz < (T)-0.5 * Lz ? dz + Lz : dz;
  }
}

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// one wave per row; f = {fx, fy, fz, pe_i} with pe_i = half of the pair energies of particle i.  status (nl_lj_forces_enqueue,
// which does not wait for the build): the build's status word; a list whose build failed gives NaN forces.
template <typename T, bool HALF, typename OFF, bool TRI>
__global__ void __launch_bounds__(256) k_lj(const T* __restrict__ q, int32_t stride, const OFF* __restrict__ kp,
                                            const int32_t* __restrict__ list, int32_t n, T eps4, T sig2, T rcf2,
                                            T* __restrict__ f, T Lx, T Ly, T Lz, const uint32_t* __restrict__ status,
                                            T xy, T xz, T yz) {
  const int32_t row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= n) return;
  if (status && *status != 0u) {  // (uniform: every row of the launch takes this branch)
    if (lane == 0) {
      const T nan = (T)NAN;
      f[(size_t)row * 4 + 0] = nan, f[(size_t)row * 4 + 1] = nan, f[(size_t)row * 4 + 2] = nan, f[(size_t)row * 4 + 3] = nan;
    }
    return;
  }
  T xi, yi, zi;
  load_xyz(q, stride, row, xi, yi, zi);
  T ax = 0, ay = 0, az = 0, ae = 0;
  const OFF b = kp[row], e = kp[row + 1];
  for (OFF k = b + lane; k < e; k += 64) {
    const int32_t j = list[k];
    T xj, yj, zj;
    load_xyz(q, stride, j, xj, yj, zj);
    T fx, fy, fz, pe;
    bool in;
    T dx = xi - xj, dy = yi - yj, dz = zi - zj;
    // minimum-image list (nl_set_periodic_axes): on a periodic axis (L > 0) the pair is taken at the image the list
    // found it at
    lj_image<T, TRI>(dx, dy, dz, Lx, Ly, Lz, xy, xz, yz);
    lj_pair<T>(dx, dy, dz, eps4, sig2, rcf2, fx, fy, fz, pe, in);
    ax += fx, ay += fy, az += fz, ae += (T)0.5 * pe;
    if (HALF && in) {  // Newton's third law: the partner's share
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
int lj_launch(nl_handle_t h, const void* q_dev, int32_t stride, double eps, double sigma, double rc_force, void* f_dev,
              hipStream_t s, const uint32_t* status = nullptr) {
  const int32_t n = h->n;
  const T eps4 = (T)(4.0 * eps), sig2 = (T)(sigma * sigma), rcf2 = (T)(rc_force * rc_force);
  const int32_t nbw = (int32_t)(((int64_t)n * 64 + 255) / 256);
  if (n == 0) return NL_OK;
  // box lengths for the minimum image on the axes of the list's build; 0 = open axis (the reference's distances,
  // neighlist_cpu.hpp:219-223)
  // (the build's box, BuildPlan::box, and its tilt: triclinic instances where it has one)
  const Box& b = h->plan.box;
  const T Lx = (h->plan.pbc & 1) ? (T)b.L[0] : (T)0, Ly = (h->plan.pbc & 2) ? (T)b.L[1] : (T)0, Lz = (h->plan.pbc & 4) ? (T)b.L[2] : (T)0;
  const T xy = (T)b.xy, xz = (T)b.xz, yz = (T)b.yz;
  auto launch = [&](auto half, auto tri) {
    hipLaunchKernelGGL((k_lj<T, decltype(half)::value, OFF, decltype(tri)::value>), dim3(nbw), dim3(256), 0, s, static_cast<const T*>(q_dev),
                       stride, static_cast<const OFF*>(h->key_pointer), h->list, n, eps4, sig2, rcf2, static_cast<T*>(f_dev), Lx, Ly, Lz,
                       status, xy, xz, yz);
  };
  if (!h->plan.full) HIPCHK(h, hipMemsetAsync(f_dev, 0, sizeof(T) * 4 * (size_t)n, s));
  if (h->plan.tilt) h->plan.full ? launch(std::false_type(), std::true_type()) : launch(std::true_type(), std::true_type());
  else h->plan.full ? launch(std::false_type(), std::false_type()) : launch(std::true_type(), std::false_type());
  HIPCHK(h, hipGetLastError());
  return NL_OK;
}

}  // namespace

extern "C" int nl_lj_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma,
                            double rc_force, void* f_dev, void* stream) {
  if (!h || !q_dev || !f_dev || (q_stride != 3 && q_stride != 4) || !(rc_force > 0) || !(sigma > 0)) return fail(h, NL_ERR_ARG);
  int rc = nl_synchronize(h);  // the list must be complete (and its build must have succeeded)
  if (rc) return rc;
  if (h->args.slab || h->n_rows != h->n) return fail(h, NL_ERR_STATE);  // ids must index q
  if (rc_force > h->rc) return fail(h, NL_ERR_ARG);                   // the list does not reach that far
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (h->plan.wide)
    return h->dtype == NL_F32 ? lj_launch<float, int64_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s)
                              : lj_launch<double, int64_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s);
  return h->dtype == NL_F32 ? lj_launch<float, int32_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s)
                            : lj_launch<double, int32_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s);
}

// nl_lj_forces without the wait: stream-ordered behind the update (or completed build) whose list it reads.
extern "C" int nl_lj_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma,
                                    double rc_force, void* f_dev, void* stream) {
  if (!h || !q_dev || !f_dev || (q_stride != 3 && q_stride != 4) || !(rc_force > 0) || !(sigma > 0)) return fail(h, NL_ERR_ARG);
  if (!(rc_force <= h->rc - h->skin)) return fail(h, NL_ERR_ARG);  // beyond what a list reused within the skin guarantees
  hipStream_t s = (hipStream_t)stream;
  if (!h->pending && !h->built) return fail(h, NL_ERR_STATE);  // no build, or one the host has seen fail
  // a pending build must be an update's (a plain asynchronous build may still need finish() to complete its list) and
  // enqueued on this stream
  if (h->pending && (!h->last_update || s != h->last_stream)) return fail(h, NL_ERR_STATE);
  if (h->args.slab || h->n_rows != h->n) return fail(h, NL_ERR_STATE);  // ids must index q
  HIPCHK(h, hipSetDevice(h->device));
  if (h->plan.wide)
    return h->dtype == NL_F32 ? lj_launch<float, int64_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s, h->status)
                              : lj_launch<double, int64_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s, h->status);
  return h->dtype == NL_F32 ? lj_launch<float, int32_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s, h->status)
                            : lj_launch<double, int32_t>(h, q_dev, q_stride, epsilon, sigma, rc_force, f_dev, s, h->status);
}
