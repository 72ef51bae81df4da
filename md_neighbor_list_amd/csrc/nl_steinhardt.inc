// nl_steinhardt.inc -- Steinhardt bond-orientational order parameters from the full list of the last build (DESIGN.md section
// 8z): q_l, w_l (normalised) and their neighbour-averaged forms (Lechner-Dellago) of every particle, for one degree l per call.
// The rule is stated at nl_set_steinhardt in include/nl_hip.h.  The first consumer that is no force field and writes no totals:
// two kernels on the persistent grid of 4-wave blocks, one wave per centre row,
//   k_stein_qlm   walks the row with lj_row_pairs; a lane whose entry is a neighbour (0 < r2 < X) evaluates Y_lm of its bond for
//                 m = 0 .. l -- the m loop is unrolled to NL_STEIN_MAX_L + 1 under the uniform test m <= l, so that the lane's
//                 2 (l + 1) sums are registers although l is a run-time argument; the degree recurrence inside is a run-time
//                 loop over coefficients that come through the scalar cache.  One wave_sum per sum and row (not per trip of the
//                 walk), lane m keeps q_lm and writes it with N_b;
//   k_stein_out   lane m reads q_lm of the row; q_l from one wave_sum; w_l from the row's q_lm of m = -l .. l in the wave's LDS
//                 strip, the (2 l + 1)^2 terms (m1, m2) of the 3j table (staged into LDS once per block) dealt to the lanes.  With
//                 `average` a second walk of the row gathers the neighbours' q_lm into the same unrolled registers, and the same
//                 two formulas run on the averaged q_lm.
// No atomic anywhere: a row's values are written by its own wave, so two calls on one list write the same bytes.
// The pieces are those of nl_consumer.inc (lj_row_pairs, grid_rows, consumer_call, list_reach, first_call_scratch), hist_edge of
// nl_histogram.inc and sqrt_t of nl_sw.inc.  Included at the end of nl_api.hip, behind nl_histogram.inc.

namespace {

constexpr int STEIN_M = NL_STEIN_MAX_L + 1;      // m = 0 .. l
constexpr int STEIN_W = 2 * NL_STEIN_MAX_L + 1;  // m = -l .. l
constexpr int STEIN_BLOCKS = 2048;               // the most blocks of either kernel (the grid of k_pair_hist)
// st_tab: the recurrence table [l + 1][l + 1] {A, B} and the 3j table [2 l + 1][2 l + 1] behind it, in T, sized for the largest l
constexpr size_t STEIN_TAB = (size_t)STEIN_M * STEIN_M * 2 + (size_t)STEIN_W * STEIN_W;
static_assert(STEIN_M <= WAVE, "lane m keeps q_lm");

// What a launch needs beside LjArgs.  rec[(m (l + 1) + k)] = {A_km, B_km} for k > m and {S_m, 0} at k = m.
template <typename T> struct SteinArgs {
  int32_t l, average, has_w;
  double r_max;
  T c_l;  // 4 pi / (2 l + 1)
  const T* __restrict__ rec;
  const T* __restrict__ w3j;
  T* qlm;        // [n][l + 1][2]
  int32_t* nb;   // [n]
  T* __restrict__ out;  // [n][4]
};

// The sums of a row's wave: lane m keeps (re, im) = the wave's totals of sr[m], si[m]; the other lanes 0.
template <typename T>
__device__ __forceinline__ void stein_lane_m(const T (&sr)[STEIN_M], const T (&si)[STEIN_M], int32_t l, int32_t lane, T& re, T& im) {
  re = im = (T)0;
#pragma unroll
  for (int m = 0; m < STEIN_M; m++) {
    if (m <= l) {  // (uniform)
      const T tr = wave_sum(sr[m]), ti = wave_sum(si[m]);
      if (lane == m) re = tr, im = ti;
    }
  }
}

template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_stein_qlm(LjArgs<T, OFF> a, SteinArgs<T> g) {
  const int32_t l = g.l, nm = l + 1;
  const T X = hist_edge<T>(1, g.r_max, 1);
  const LjScalars<T> none = {(T)0, (T)0, (T)0};
  const bool dead = a.status && *a.status != 0u;  // (uniform over the launch) a failed list is not read
  grid_rows(a.n, [&](int32_t row, int32_t lane) {
    T sr[STEIN_M], si[STEIN_M];
#pragma unroll
    for (int m = 0; m < STEIN_M; m++) sr[m] = si[m] = (T)0;
    int32_t cnt = 0;
    if (!dead)
      lj_row_pairs<T, OFF, TRI>(a, none, row, lane, [&](int32_t, LjPartner, T dx, T dy, T dz, T, T, T, T, bool) {
        const T r2 = (dx * dx + dy * dy) + dz * dz;
        if (!(r2 < X && r2 > (T)0)) return;
        cnt++;
        const T ir = (T)1 / sqrt_t(r2);
        const T x = (-dx) * ir, y = (-dy) * ir, z = (-dz) * ir;  // u = (r_j - r_i) / r
        T cr = (T)1, ci = (T)0;                                  // (x + i y)^m
#pragma unroll
        for (int m = 0; m < STEIN_M; m++) {
          if (m <= l) {  // (uniform)
            if (m > 0) {
              const T nr = cr * x - ci * y, ni = cr * y + ci * x;
              cr = nr, ci = ni;
            }
            const T* __restrict__ rc = g.rec + (size_t)(m * nm) * 2;
            T p1 = rc[2 * m], p2 = (T)0;
            for (int32_t k = m + 1; k <= l; k++) {
              const T p = (rc[2 * k] * z) * p1 - rc[2 * k + 1] * p2;
              p2 = p1, p1 = p;
            }
            sr[m] += p1 * cr, si[m] += p1 * ci;
          }
        }
      });
    const int32_t nbr = wave_sum(cnt);
    T re, im;
    stein_lane_m(sr, si, l, lane, re, im);
    const T fn = (T)nbr;  // (N_b = 0: 0 / 0, the NaN of a centre without neighbours)
    if (lane <= l) {
      T* o = g.qlm + ((size_t)row * nm + lane) * 2;
      o[0] = dead ? (T)NAN : re / fn, o[1] = dead ? (T)NAN : im / fn;
    }
    if (lane == 0) g.nb[row] = nbr;
  });
}

// The LDS of a block of k_stein_out: the 3j table and a strip of q_lm, m = -l .. l, per wave.
template <typename T> struct SteinLds {
  T w[STEIN_W * STEIN_W];
  T q[4][STEIN_W][2];
};

// {q_l, w_l} from the q_lm the lanes m = 0 .. l hold ((re, im); the other lanes hold 0).  Called by the whole wave.
template <typename T>
__device__ __forceinline__ void stein_columns(const SteinArgs<T>& g, SteinLds<T>& lds, int32_t lane, T re, T im, T& ql, T& wl) {
  const int32_t l = g.l, nw = 2 * l + 1, wave = threadIdx.x >> 6;
  const T v = re * re + im * im;
  const T s = wave_sum(lane == 0 ? v : v + v);  // sum over m = -l .. l of |q_lm|^2
  ql = sqrt_t(g.c_l * s);
  wl = (T)NAN;
  if (!g.has_w) return;  // (uniform)
  T(*q)[2] = lds.q[wave];
  if (lane <= l) {
    const T sg = (lane & 1) ? (T)-1 : (T)1;  // q_{l,-m} = (-1)^m conj(q_lm)
    q[l + lane][0] = re, q[l + lane][1] = im;
    q[l - lane][0] = sg * re, q[l - lane][1] = -(sg * im);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  T acc = (T)0;
  for (int32_t t = lane; t < nw * nw; t += WAVE) {
    const int32_t i1 = t / nw, i2 = t - i1 * nw, i3 = 3 * l - i1 - i2;  // m3 = -m1 - m2
    if (i3 < 0 || i3 >= nw) continue;
    const T pr = q[i1][0] * q[i2][0] - q[i1][1] * q[i2][1], pi = q[i1][0] * q[i2][1] + q[i1][1] * q[i2][0];
    acc += lds.w[t] * (pr * q[i3][0] - pi * q[i3][1]);
  }
  __builtin_amdgcn_wave_barrier();  // (the next writes of the strip stay behind these reads)
  wl = wave_sum(acc) / (s * sqrt_t(s));
}

template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_stein_out(LjArgs<T, OFF> a, SteinArgs<T> g) {
  __shared__ SteinLds<T> lds;
  const int32_t l = g.l, nm = l + 1, nw = 2 * l + 1;
  if (g.has_w) {
    for (int32_t t = threadIdx.x; t < nw * nw; t += STAGE_THREADS) lds.w[t] = g.w3j[t];
  }
  __syncthreads();
  const T X = hist_edge<T>(1, g.r_max, 1);
  const LjScalars<T> none = {(T)0, (T)0, (T)0};
  const T nan = (T)NAN;
  const bool dead = a.status && *a.status != 0u;  // (uniform over the launch)
  grid_rows(a.n, [&](int32_t row, int32_t lane) {
    T* o = g.out + (size_t)row * 4;
    if (dead) {
      if (lane < 4) o[lane] = nan;
      return;
    }
    T re = (T)0, im = (T)0;
    if (lane <= l) {
      const T* qi = g.qlm + ((size_t)row * nm + lane) * 2;
      re = qi[0], im = qi[1];
    }
    T ql, wl, qa = nan, wa = nan;
    stein_columns(g, lds, lane, re, im, ql, wl);
    if (g.average) {  // (uniform)
      T sr[STEIN_M], si[STEIN_M];
#pragma unroll
      for (int m = 0; m < STEIN_M; m++) sr[m] = si[m] = (T)0;
      lj_row_pairs<T, OFF, TRI>(a, none, row, lane, [&](int32_t j, LjPartner, T dx, T dy, T dz, T, T, T, T, bool) {
        const T r2 = (dx * dx + dy * dy) + dz * dz;
        if (!(r2 < X && r2 > (T)0)) return;
        const T* qj = g.qlm + (size_t)j * nm * 2;
#pragma unroll
        for (int m = 0; m < STEIN_M; m++) {
          if (m <= l) sr[m] += qj[2 * m], si[m] += qj[2 * m + 1];  // (uniform)
        }
      });
      T ar, ai;
      stein_lane_m(sr, si, l, lane, ar, ai);
      const T d = (T)(g.nb[row] + 1);
      if (lane <= l) ar = (re + ar) / d, ai = (im + ai) / d;
      stein_columns(g, lds, lane, ar, ai, qa, wa);
    }
    if (lane == 0) o[0] = ql, o[1] = wl, o[2] = qa, o[3] = wa;
  });
}

// ---- host side
// The scratch of the family: q_lm [n_max + 16][l + 1][2] of T and N_b [n_max + 16] behind it.  The first-call rule of the totals
// (first_call_scratch); regrown by the first call after an nl_initialize that changed n_max, or after a setting with a larger l.
size_t stein_qlm_bytes(nl_handle_t h, int32_t l) { return ((size_t)h->n_max + 16) * (size_t)(l + 1) * 2 * (h->dtype == NL_F32 ? 4 : 8); }
int stein_scratch(nl_handle_t h, hipStream_t s) {
  if (h->st_part && (h->st_cap_l < h->st_l || h->st_cap_n != h->n_max)) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(h, hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(h, NL_ERR_STATE);
    HIPCHK(h, hipDeviceSynchronize());  // (a call in flight may still write the old one)
    h->st_part.release();
    h->st_last_l = 0;
  }
  if (h->st_part) return NL_OK;
  if (int rc = first_call_scratch(h, h->st_part, stein_qlm_bytes(h, h->st_l) + 4 * ((size_t)h->n_max + 16), s)) return rc;
  h->st_cap_l = h->st_l, h->st_cap_n = h->n_max;
  return NL_OK;
}
int32_t* stein_nb(nl_handle_t h) { return reinterpret_cast<int32_t*>(static_cast<char*>(h->st_part.get()) + stein_qlm_bytes(h, h->st_cap_l)); }

int stein_launch(nl_handle_t h, const void* q_dev, int32_t stride, int average, void* out_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  if (int rc = stein_scratch(h, s)) return rc;
  const int32_t l = h->st_l;
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, STEIN_BLOCKS);
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    const T* tab = static_cast<const T*>(h->st_tab.get());
    const SteinArgs<T> g = {l, average ? 1 : 0, h->st_w ? 1 : 0, h->st_rmax, (T)(4.0 * M_PI / (double)(2 * l + 1)), tab,
                            tab + (size_t)STEIN_M * STEIN_M * 2, static_cast<T*>(h->st_part.get()), stein_nb(h), static_cast<T*>(out_dev)};
    with_flag(h->plan.tilt, [&](auto tri) {
      constexpr bool R = decltype(tri)::value;
      hipLaunchKernelGGL((k_stein_qlm<T, OFF, R>), dim3(nblk), dim3(STAGE_THREADS), 0, s, a, g);
      hipLaunchKernelGGL((k_stein_out<T, OFF, R>), dim3(nblk), dim3(STAGE_THREADS), 0, s, a, g);
    });
    HIPCHK(h, hipGetLastError());
    h->st_last_l = l;
    return NL_OK;
  });
}

// A setting; a whole single-device FULL list (a row must hold every neighbour of its centre, for its own sum and for the
// average, which also needs q_lm of every partner: slab lists are refused, local-index ones included); r_max within what the list
// guarantees -- a pair of types with rc_ab = 0 is no neighbour pair and asks for nothing.
int stein_reach(nl_handle_t h, double skin) {
  if (h->st_l == 0) return fail(h, NL_ERR_STATE);
  if (!h->plan.full || h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  return h->st_rmax <= list_reach(h, /*skip_zero=*/true) - skin ? NL_OK : fail(h, NL_ERR_ARG);
}

int stein_call(nl_handle_t h, const void* q_dev, int32_t q_stride, int average, void* out_dev, void* stream, bool enqueue) {
  return consumer_call(
      h, q_dev, q_stride, out_dev, true, stream, enqueue, [&](double skin) { return stein_reach(h, skin); },
      [&](hipStream_t s, const uint32_t* status) { return stein_launch(h, q_dev, q_stride, average, out_dev, s, status); });
}

// The tables of a degree l in double: {A_km, B_km} of the recurrence in the degree k and the start S_m at k = m, then w3j.
//   A_km = sqrt((4 k^2 - 1) / (k^2 - m^2)),  B_km = A_km sqrt(((k - 1)^2 - m^2) / (4 (k - 1)^2 - 1)),
//   S_m = (-1)^m sqrt((2 m + 1) / (4 pi) prod_{i = 1 .. m} (2 i - 1) / (2 i)).
template <typename T> void stein_tables(int32_t l, const double* w3j, T* out) {
  const int32_t nm = l + 1, nw = 2 * l + 1;
  for (int32_t m = 0; m <= l; m++) {
    double pr = 1.0;
    for (int32_t i = 1; i <= m; i++) pr *= (double)(2 * i - 1) / (double)(2 * i);
    const double sm = ((m & 1) ? -1.0 : 1.0) * std::sqrt((double)(2 * m + 1) / (4.0 * M_PI) * pr);
    for (int32_t k = 0; k <= l; k++) {
      double A = 0.0, B = 0.0;
      if (k == m) A = sm;
      if (k > m) {
        A = std::sqrt((double)(4 * k * k - 1) / (double)(k * k - m * m));
        B = A * std::sqrt((double)((k - 1) * (k - 1) - m * m) / (double)(4 * (k - 1) * (k - 1) - 1));
      }
      out[(size_t)(m * nm + k) * 2] = (T)A, out[(size_t)(m * nm + k) * 2 + 1] = (T)B;
    }
  }
  T* w = out + (size_t)STEIN_M * STEIN_M * 2;
  for (int32_t t = 0; t < nw * nw; t++) w[t] = w3j ? (T)w3j[t] : (T)0;
}

}  // namespace

extern "C" {

int nl_set_steinhardt(nl_handle_t h, int32_t l, double r_max, const double* w3j_host) {
  if (!h) return NL_ERR_ARG;
  if (l == 0) {  // clear (the buffers stay: a captured graph may still read them)
    h->st_l = 0, h->st_w = false, h->st_rmax = 0;
    return NL_OK;
  }
  if (l < 1 || l > NL_STEIN_MAX_L || !(r_max > 0) || !std::isfinite(r_max)) return fail(h, NL_ERR_ARG);
  if (w3j_host)
    for (int32_t t = 0; t < (2 * l + 1) * (2 * l + 1); t++)
      if (!std::isfinite(w3j_host[t])) return fail(h, NL_ERR_ARG);
  HIPCHK(h, hipSetDevice(h->device));
  const bool f32 = h->dtype == NL_F32;
  const size_t bytes = STEIN_TAB * (f32 ? 4 : 8);
  std::vector<char> tab(bytes);
  if (f32) stein_tables(l, w3j_host, reinterpret_cast<float*>(tab.data()));
  else stein_tables(l, w3j_host, reinterpret_cast<double*>(tab.data()));
  HIPCHK(h, hipDeviceSynchronize());  // (the device may still run a call that reads the old tables)
  if (!h->st_tab)  // (no build touches it: side_alloc's kind; sized for the largest l, so that it is allocated once)
    if (int rc = side_alloc(h, h->st_tab, bytes)) return rc;
  HIPCHK(h, hipMemcpy(h->st_tab, tab.data(), bytes, hipMemcpyHostToDevice));
  h->st_l = l, h->st_rmax = r_max, h->st_w = w3j_host != nullptr;
  return NL_OK;
}

int nl_get_steinhardt(nl_handle_t h, int32_t* l, double* r_max, int32_t* has_w) {
  if (!h) return NL_ERR_ARG;
  if (h->st_l == 0) return fail(h, NL_ERR_STATE);
  if (l) *l = h->st_l;
  if (r_max) *r_max = h->st_rmax;
  if (has_w) *has_w = h->st_w ? 1 : 0;
  return NL_OK;
}

int nl_steinhardt(nl_handle_t h, const void* q_dev, int32_t q_stride, int average, void* out_dev, void* stream) {
  return stein_call(h, q_dev, q_stride, average, out_dev, stream, false);
}
int nl_steinhardt_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, int average, void* out_dev, void* stream) {
  return stein_call(h, q_dev, q_stride, average, out_dev, stream, true);
}

int nl_steinhardt_get_qlm(nl_handle_t h, const void** qlm_dev, const int32_t** count_dev, int32_t* n, int32_t* l) {
  if (!h || !qlm_dev || !count_dev || !n || !l) return fail(h, NL_ERR_ARG);
  if (!h->st_part || h->st_last_l == 0 || h->st_cap_n != h->n_max) return fail(h, NL_ERR_STATE);
  *qlm_dev = h->st_part.get();
  *count_dev = stein_nb(h);
  *n = h->n_rows;
  *l = h->st_last_l;
  return NL_OK;
}

}  // extern "C"
