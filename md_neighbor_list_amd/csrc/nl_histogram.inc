// nl_histogram.inc -- the pair-distance histogram of the last build's list (DESIGN.md section 8m): the counts behind g(r),
// one histogram for everybody (nl_pair_histogram) or one per unordered pair of types (nl_pair_histogram_typed), added to
// uint64 counters of the caller on the device.  The rule is stated at nl_pair_histogram in include/nl_hip.h.
// A third consumer on the shared walk of section 8l: the rows and the separations are lj_row_pairs' (lj_image; the values
// of lj_pair are ignored and the compiler drops them), a particle's type and a pair's slot are type_of and pair_slot, the entry
// path is consumer_call's with the histogram's own arguments and reach over list_reach (hist_call; DESIGN.md section 8q).
// Integer counters only: the answer is exact, the same for a half and a full build bit for bit, and the same every call.
// Included at the end of nl_api.hip, behind nl_virial.inc.

namespace {

constexpr int HIST_BLOCKS = 2048;  // the most blocks of k_pair_hist (the grid of k_lj_virial)
static_assert(STAGE_THREADS == 4 * WAVE, "k_pair_hist deals rows to the 4 waves of a block");
// the largest launch: NL_HIST_LDS_COUNTERS counters and the edges E_1 .. E_nbins of a double list in 64 KB of LDS
static_assert(NL_HIST_LDS_COUNTERS * sizeof(uint64_t) + NL_HIST_MAX_BINS * sizeof(double) <= 65536, "LDS of k_pair_hist");
// ... and one slot always fits, so the untyped kernels have no other path
static_assert(NL_HIST_MAX_BINS <= NL_HIST_LDS_COUNTERS, "k_pair_hist counts in LDS");

// What a launch needs beside LjArgs.
struct HistArgs {
  double r_max;
  int32_t nbins, ntypes, full;
  const int32_t* __restrict__ types;  // typed: the handle's type table
  unsigned long long* __restrict__ hist;
};

// E_k, k >= 1: the largest T <= e_k e_k with e_k = (k r_max) / nbins in double -- the rounding of Grid::rc2 (floor_to_float).
template <typename T> __device__ __forceinline__ T hist_edge(int32_t k, double r_max, int32_t nbins) {
  const double e = ((double)k * r_max) / (double)nbins;
  const double sq = e * e;
  if constexpr (sizeof(T) == 8) {
    return sq;
  } else {
    float f = (float)sq;
    if ((double)f > sq) f = __uint_as_float(__float_as_uint(f) - 1u);  // (f > 0 here: the next float towards 0)
    return f;
  }
}

// One wave per row, the rows dealt to the waves of the grid in turn (as lj_virial_rows).  LDS: the counters of the block
// live in LDS (nslots * nbins <= NL_HIST_LDS_COUNTERS) and go to hist at its end; otherwise every entry goes to hist.  The
// choice is an instance, not a branch: with both adds in one body the compiler merges them into one flat atomic on a
// selected pointer.  Dynamic LDS of a block:
//   cnt[LDS ? nslots * nbins : 0] uint64, then edge[nbins] of T with edge[k - 1] = E_k (E_0 = 0 is not stored).
// An entry's bin: a guess from sqrtf(r2) nbins / r_max, then steps along the table until E_b <= r2 < E_{b+1}; the table alone
// decides.  r2 >= E_nbins and NaN leave before the steps (!(r2 < E_nbins)), so both loops end: E_0 = 0 <= r2 stops the
// way down, r2 < E_nbins the way up.
// A failed list (status, the enqueue variants) is not read and nothing is added.
template <typename T, typename OFF, bool TRI, bool TYPED, bool LDS>
__device__ __forceinline__ void pair_hist_rows(const LjArgs<T, OFF>& a, const HistArgs& g) {
  extern __shared__ unsigned long long hist_lds[];
  const int32_t nbins = g.nbins;
  const int32_t nslots = TYPED ? g.ntypes * (g.ntypes + 1) / 2 : 1;
  const int32_t ncnt = LDS ? nslots * nbins : 0;
  unsigned long long* cnt = hist_lds;
  T* edge = reinterpret_cast<T*>(hist_lds + ncnt);
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t k = threadIdx.x; k < ncnt; k += STAGE_THREADS) cnt[k] = 0ull;
  for (int32_t k = threadIdx.x; k < nbins; k += STAGE_THREADS) edge[k] = hist_edge<T>(k + 1, g.r_max, nbins);
  __syncthreads();
  const T top = edge[nbins - 1];
  const float scale = (float)((double)nbins / g.r_max);
  const bool live = !(a.status && *a.status != 0u);  // (uniform over the launch)
  const LjScalars<T> none = {(T)0, (T)0, (T)0};
  if constexpr (TYPED) __builtin_assume(g.types != nullptr);  // (type_of asks; a typed launch has the table)
  for (int32_t row = (int32_t)blockIdx.x * 4 + wave; live && row < a.n; row += (int32_t)gridDim.x * 4) {
    const int32_t ti = TYPED ? type_of(g.types, row, g.ntypes) : 0;
    lj_row_pairs<T, OFF, TRI>(a, none, row, lane, [&](int32_t j, LjPartner w, T dx, T dy, T dz, T, T, T, T, bool) {
      // a pair stored twice counts once: a full list's in the row of the smaller id, one that crosses a cut of a local-id
      // slab build (both ranks store it, half or full) on the rank LjPartner::first names
      if (w.ghost ? !w.first : (g.full && j <= row)) return;
      const T r2 = (dx * dx + dy * dy) + dz * dz;
      if (!(r2 < top)) return;  // beyond r_max, or NaN
      int32_t b = min((int32_t)(sqrtf((float)r2) * scale), nbins - 1);
      while (b > 0 && r2 < edge[b - 1]) b--;
      while (r2 >= edge[b]) b++;
      const int32_t slot = TYPED ? pair_slot(ti, type_of(g.types, j, g.ntypes), g.ntypes) : 0;
      const int32_t at = slot * nbins + b;
      if constexpr (LDS) atomicAdd(&cnt[at], 1ull);
      else atomicAdd(&g.hist[at], 1ull);
    });
  }
  if constexpr (!LDS) return;
  __syncthreads();
  for (int32_t k = threadIdx.x; k < ncnt; k += STAGE_THREADS) {
    const unsigned long long v = cnt[k];
    if (v) atomicAdd(&g.hist[k], v);
  }
}

template <typename T, typename OFF, bool TRI>
__global__ void __launch_bounds__(STAGE_THREADS) k_pair_hist(LjArgs<T, OFF> a, HistArgs g) {
  pair_hist_rows<T, OFF, TRI, false, true>(a, g);
}
template <typename T, typename OFF, bool TRI, bool LDS>
__global__ void __launch_bounds__(STAGE_THREADS) k_pair_hist_typed(LjArgs<T, OFF> a, HistArgs g) {
  pair_hist_rows<T, OFF, TRI, true, LDS>(a, g);
}

int hist_launch(nl_handle_t h, const void* q_dev, int32_t stride, double r_max, int32_t nbins, bool typed, uint64_t* hist_dev,
                hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  const int32_t nt = typed ? h->ty_ntypes : 1;
  const int64_t ncnt = (int64_t)(nt * (nt + 1) / 2) * nbins;
  const bool lds = ncnt <= NL_HIST_LDS_COUNTERS;
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, HIST_BLOCKS);
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    const HistArgs g = {r_max, nbins, nt, h->plan.full ? 1 : 0, typed ? h->ty_types.get() : nullptr,
                        reinterpret_cast<unsigned long long*>(hist_dev)};
    const size_t bytes = (lds ? sizeof(uint64_t) * (size_t)ncnt : 0) + sizeof(T) * (size_t)nbins;
    auto launch = [&](auto tri) {
      constexpr bool R = decltype(tri)::value;
      if (typed && lds) hipLaunchKernelGGL((k_pair_hist_typed<T, OFF, R, true>), dim3(nblk), dim3(STAGE_THREADS), bytes, s, a, g);
      else if (typed) hipLaunchKernelGGL((k_pair_hist_typed<T, OFF, R, false>), dim3(nblk), dim3(STAGE_THREADS), bytes, s, a, g);
      else hipLaunchKernelGGL((k_pair_hist<T, OFF, R>), dim3(nblk), dim3(STAGE_THREADS), bytes, s, a, g);
    };
    with_flag(h->plan.tilt, launch);
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

// The histogram cannot see further than the list: r_max within every cut-off the list was built with, less the skin for
// a list that may be reused.  Untyped: rc, and with a type table every rc_ab (a pair of types with rc_ab = 0 is not in the
// list at all: refused).  Typed: every rc_ab > 0; a pair with rc_ab = 0 has no entries and its slot stays as it was.
int hist_reach(nl_handle_t h, double r_max, bool typed, double skin) {
  if (typed && !h->ty_types) return fail(h, NL_ERR_STATE);
  return r_max <= list_reach(h, typed) - skin ? NL_OK : fail(h, NL_ERR_ARG);
}

// The four entry points: consumer_call with the histogram's arguments and reach.
int hist_call(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins, uint64_t* hist_dev, void* stream,
              bool enqueue, bool typed) {
  return consumer_call(
      h, q_dev, q_stride, hist_dev, r_max > 0 && std::isfinite(r_max) && nbins >= 1 && nbins <= NL_HIST_MAX_BINS, stream, enqueue,
      [&](double skin) { return hist_reach(h, r_max, typed, skin); },
      [&](hipStream_t s, const uint32_t* status) { return hist_launch(h, q_dev, q_stride, r_max, nbins, typed, hist_dev, s, status); });
}

}  // namespace

extern "C" {

int nl_pair_histogram(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins, uint64_t* hist_dev,
                      void* stream) {
  return hist_call(h, q_dev, q_stride, r_max, nbins, hist_dev, stream, false, false);
}
int nl_pair_histogram_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins, uint64_t* hist_dev,
                              void* stream) {
  return hist_call(h, q_dev, q_stride, r_max, nbins, hist_dev, stream, true, false);
}
int nl_pair_histogram_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins, uint64_t* hist_dev,
                            void* stream) {
  return hist_call(h, q_dev, q_stride, r_max, nbins, hist_dev, stream, false, true);
}
int nl_pair_histogram_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins,
                                    uint64_t* hist_dev, void* stream) {
  return hist_call(h, q_dev, q_stride, r_max, nbins, hist_dev, stream, true, true);
}

}  // extern "C"
