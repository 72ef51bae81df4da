// nl_cna.inc -- common neighbour analysis from the full list of the last build (DESIGN.md section 8zb): the structure type of
// every particle (fcc, hcp, bcc, icosahedral, other) from the Honeycutt-Andersen / Faken-Jonsson signatures of its bonds, with a
// fixed cut-off or Stukowski's adaptive one.  The rule is stated at nl_cna in include/nl_hip.h.  All common neighbours of i and k
// are neighbours of i, so one row of the list and the positions hold everything a centre needs and no partner's row is read:
// one kernel on the persistent grid of 4-wave blocks, one wave per centre row,
//   1. walks the row with lj_row_pairs; the candidates (0 < r2 < X) are compacted into the wave's LDS strip {d, r2} at
//      m + lanes_below(ballot) as sw_row compacts its partners, j into the (still unused) adjacency words; the walk is finished
//      with the stores off once m passes 64, so that N_b is exact for an overflowed centre too;
//   2. ADAPTIVE: lane t ranks its candidate by (r2, j) against all m of the strip and moves it to slot rank, so that from here on
//      lane t holds the candidate of rank t and the 12-set and the 14-set are the lanes 0 .. 11 and 0 .. 13; the terms of S are
//      added in rank order, every lane the same sum, from v_readlane broadcasts;
//   3. lane k < m_set tests its d against d_m of m = 0 .. m_set - 1, broadcast from the strip, and keeps its 64-bit adjacency
//      word, which goes to LDS;
//   4. lane k: C = adj[k], ncn = popcount, nb = sum over m in C of popcount(adj[m] & C) / 2, and lc by a bit flood-fill of the
//      graph (C, bonds) -- only where (ncn, nb) is that of a counted signature, which no other value of lc can make one;
//   5. the five signature counts by ballot; lane 0 writes the type and the counts; the block's tally of the types lives in LDS
//      and goes to the summary with one integer atomic per word at the block's end (the histogram's way).
// Integers out, and no floating-point atomic: two calls write the same bytes.  No scratch on the handle.
// The pieces are those of nl_consumer.inc (LjArgs, lj_args, lj_row_pairs, grid_rows, consumer_call, list_reach), hist_edge of
// nl_histogram.inc, readlane_t and sqrt_t of nl_sw.inc.  Included at the end of nl_api.hip, behind nl_cluster.inc.

namespace {

constexpr int CNA_BLOCKS = 2048;  // the most blocks of k_cna (the grid of k_pair_hist)
static_assert(NL_CNA_MAX_NEAR == WAVE, "one candidate per lane and one bit per candidate");
static_assert(NL_CNA_OTHER == 0 && NL_CNA_FCC == 1 && NL_CNA_HCP == 2 && NL_CNA_BCC == 3 && NL_CNA_ICO == 4, "the summary's words");

// What a launch needs beside LjArgs.
struct CnaArgs {
  double r_max;
  int32_t* __restrict__ type;            // [n]
  int32_t* __restrict__ counts;          // [n][8] or nullptr
  unsigned long long* __restrict__ summary;  // [6] or nullptr
};

// The LDS of a block: per wave the strip {dx, dy, dz, r2} of 64 slots and the 64 adjacency words; the block's tally.
template <typename T> struct CnaLds {
  T x[4][WAVE], y[4][WAVE], z[4][WAVE], r2[4][WAVE];
  unsigned long long adj[4][WAVE];
  unsigned int tally[6];  // (a block meets at most n rows, below 2^31)
};
static_assert(sizeof(CnaLds<double>) <= 10 * 1024 + 64, "LDS does not limit the occupancy");

// A wave's view of it.
template <typename T> struct CnaStrip {
  T *x, *y, *z, *r2;
  unsigned long long* adj;
};

// Between a wave's writes of its strip and the reads of other lanes (and back): the wave runs in step, so this only keeps the
// compiler from moving a lane's accesses across it (stein_columns').
__device__ __forceinline__ void cna_step() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The signature counts {n421, n422, n444, n555, n666} of the set that the lanes 0 .. m_set - 1 hold (d = (dx, dy, dz) of this
// lane's member), bonds e2 < Y.  Called by the whole wave; the strip's x, y, z hold d of slot m for every m < m_set.
template <typename T>
__device__ __forceinline__ void cna_signatures(const CnaStrip<T>& st, int32_t lane, int32_t m_set, T Y, T dx, T dy, T dz, int32_t (&n)[5]) {
  // step 3: the adjacency word of this lane's member, restricted to the set
  unsigned long long mine = 0ull;
  for (int32_t m = 0; m < m_set; m++) {  // (uniform: the reads are broadcasts)
    const T ex = dx - st.x[m], ey = dy - st.y[m], ez = dz - st.z[m];
    const T e2 = (ex * ex + ey * ey) + ez * ez;
    if (e2 < Y && m != lane) mine |= 1ull << m;
  }
  const bool member = lane < m_set;
  st.adj[lane] = member ? mine : 0ull;
  cna_step();
  // step 4: the signature of the bond (centre, this lane's member)
  int32_t ncn = 0, nb = 0, lc = 0;
  if (member) {
    const unsigned long long C = mine;
    ncn = __popcll(C);
    int32_t twice = 0;
    for (unsigned long long t = C; t; t &= t - 1) twice += __popcll(st.adj[__ffsll((long long)t) - 1] & C);
    nb = twice >> 1;
    const bool counted = (ncn == 4 && (nb == 2 || nb == 4)) || (ncn == 5 && nb == 5) || (ncn == 6 && nb == 6);
    if (counted) {  // the largest number of bonds in one connected component of (C, bonds)
      unsigned long long rem = C;
      while (rem) {
        unsigned long long reach = rem & (~rem + 1ull);  // the lowest member not visited yet
        for (;;) {  // (ends: reach only grows, within C)
          unsigned long long grow = reach;
          for (unsigned long long t = reach; t; t &= t - 1) grow |= st.adj[__ffsll((long long)t) - 1] & C;
          if (grow == reach) break;
          reach = grow;
        }
        int32_t b2 = 0;
        for (unsigned long long t = reach; t; t &= t - 1) b2 += __popcll(st.adj[__ffsll((long long)t) - 1] & reach);
        lc = max(lc, b2 >> 1);
        rem &= ~reach;
      }
    }
  }
  cna_step();  // (the next writes of the adjacency words stay behind these reads)
  // step 5: the counts
  n[0] = __popcll(__ballot(ncn == 4 && nb == 2 && lc == 1));
  n[1] = __popcll(__ballot(ncn == 4 && nb == 2 && lc == 2));
  n[2] = __popcll(__ballot(ncn == 4 && nb == 4 && lc == 4));
  n[3] = __popcll(__ballot(ncn == 5 && nb == 5 && lc == 5));
  n[4] = __popcll(__ballot(ncn == 6 && nb == 6 && lc == 6));
}

__device__ __forceinline__ int32_t cna_type12(const int32_t (&n)[5]) {
  return n[0] == 12 ? NL_CNA_FCC : (n[0] == 6 && n[1] == 6) ? NL_CNA_HCP : n[3] == 12 ? NL_CNA_ICO : NL_CNA_OTHER;
}
__device__ __forceinline__ int32_t cna_type14(const int32_t (&n)[5]) { return (n[2] == 6 && n[4] == 8) ? NL_CNA_BCC : NL_CNA_OTHER; }

// Y of the adaptive sets from the terms the lanes 0 .. count - 1 hold: S in rank order, one rounding per add.
template <typename T> __device__ __forceinline__ T cna_adaptive_y(T term, int32_t count) {
  T S = readlane_t(term, 0);
  for (int32_t t = 1; t < count; t++) S += readlane_t(term, t);
  const T c = (S / (T)count) * (T)1.2071067811865475;  // K: the double nearest (1 + sqrt 2) / 2, rounded to T
  return c * c;
}

// Zeroes the summary in front of k_cna's adds; a failed list (status, the enqueue variant): -1 in every word.
__global__ void k_cna_zero(const uint32_t* __restrict__ status, unsigned long long* summary) {
  const bool dead = status && *status != 0u;
  if (threadIdx.x < 6) summary[threadIdx.x] = dead ? ~0ull : 0ull;
}

template <typename T, typename OFF, bool TRI, bool ADAPTIVE>
__global__ void __launch_bounds__(STAGE_THREADS) k_cna(LjArgs<T, OFF> a, CnaArgs g) {
  __shared__ CnaLds<T> lds;
  if (threadIdx.x < 6) lds.tally[threadIdx.x] = 0u;
  __syncthreads();
  const int32_t wave = threadIdx.x >> 6;
  const CnaStrip<T> st = {lds.x[wave], lds.y[wave], lds.z[wave], lds.r2[wave], lds.adj[wave]};
  const T X = hist_edge<T>(1, g.r_max, 1);
  const LjScalars<T> none = {(T)0, (T)0, (T)0};
  const bool dead = a.status && *a.status != 0u;  // (uniform over the launch) a failed list is not read
  grid_rows(a.n, [&](int32_t row, int32_t lane) {
    if (dead) {
      if (lane == 0) g.type[row] = -1;
      if (g.counts && lane < 8) g.counts[(size_t)row * 8 + lane] = -1;
      return;
    }
    // step 1: the candidates, compacted
    int32_t m = 0;
    lj_row_pairs<T, OFF, TRI>(a, none, row, lane, [&](int32_t j, LjPartner, T dx, T dy, T dz, T, T, T, T, bool) {
      const T r2 = (dx * dx + dy * dy) + dz * dz;
      const bool in = r2 < X && r2 > (T)0;
      const uint64_t hit = __ballot(in);  // (of the lanes still in the walk: the others hold no entry)
      const int32_t at = m + (int32_t)lanes_below(hit);
      if (in && at < WAVE) st.x[at] = dx, st.y[at] = dy, st.z[at] = dz, st.r2[at] = r2, st.adj[at] = (unsigned long long)(uint32_t)j;
      m += (int32_t)__popcll(hit);
    });
    m = __builtin_amdgcn_readfirstlane(m);  // (lane 0 is in every chunk of the walk)
    cna_step();
    int32_t type = NL_CNA_OTHER, m_set = 0, flags = 0;
    int32_t n[5] = {0, 0, 0, 0, 0};
    if (m > WAVE) {  // (uniform) more candidates than lanes: no analysis
      flags = 1;
    } else {
      const bool live = lane < m;
      T dx = live ? st.x[lane] : (T)0, dy = live ? st.y[lane] : (T)0, dz = live ? st.z[lane] : (T)0;
      T r2 = live ? st.r2[lane] : (T)0;
      (void)r2;
      if constexpr (!ADAPTIVE) {
        cna_step();  // (these reads in front of the adjacency words' writes, which lie where j was)
        m_set = m;
        cna_signatures(st, lane, m_set, X, dx, dy, dz, n);
        type = m == 12 ? cna_type12(n) : m == 14 ? cna_type14(n) : NL_CNA_OTHER;
      } else if (m >= 12) {  // (uniform)
        // step 2: rank by (r2, j), and the strip into rank order
        const uint32_t j = live ? (uint32_t)st.adj[lane] : 0u;
        int32_t rank = 0;
        for (int32_t u = 0; u < m; u++) {  // (uniform: broadcasts)
          const T ru = st.r2[u];
          const uint32_t ju = (uint32_t)st.adj[u];
          rank += (ru < r2 || (ru == r2 && ju < j)) ? 1 : 0;
        }
        cna_step();
        if (live) st.x[rank] = dx, st.y[rank] = dy, st.z[rank] = dz, st.r2[rank] = r2;
        cna_step();
        dx = live ? st.x[lane] : (T)0, dy = live ? st.y[lane] : (T)0, dz = live ? st.z[lane] : (T)0, r2 = live ? st.r2[lane] : (T)0;
        const T root = sqrt_t(r2);
        m_set = 12;
        cna_signatures(st, lane, m_set, cna_adaptive_y(root, 12), dx, dy, dz, n);
        type = cna_type12(n);
        if (type == NL_CNA_OTHER && m >= 14) {  // (uniform)
          m_set = 14;
          cna_signatures(st, lane, m_set, cna_adaptive_y(lane < 8 ? sqrt_t(r2 / (T)0.75) : root, 14), dx, dy, dz, n);
          type = cna_type14(n);
        }
      }
      cna_step();  // (the next row's writes stay behind this row's reads)
    }
    if (lane == 0) {
      g.type[row] = type;
      if (g.summary) {
        atomicAdd(&lds.tally[type], 1u);
        if (flags) atomicAdd(&lds.tally[5], 1u);
      }
    }
    if (g.counts && lane < 8) {
      const int32_t v = lane == 0 ? m : lane == 1 ? m_set : lane == 2 ? n[0] : lane == 3 ? n[1] : lane == 4 ? n[2] : lane == 5 ? n[3]
                        : lane == 6 ? n[4] : flags;
      g.counts[(size_t)row * 8 + lane] = v;
    }
  });
  if (!g.summary || dead) return;  // (uniform)
  __syncthreads();
  if (threadIdx.x < 6 && lds.tally[threadIdx.x]) atomicAdd(&g.summary[threadIdx.x], (unsigned long long)lds.tally[threadIdx.x]);
}

// ---- host side
int cna_launch(nl_handle_t h, const void* q_dev, int32_t stride, int mode, double r_max, int32_t* type_dev, int32_t* counts_dev,
               int64_t* summary_dev, hipStream_t s, const uint32_t* status) {
  const int32_t n = h->n_rows;
  if (n == 0) return NL_OK;
  const CnaArgs g = {r_max, type_dev, counts_dev, reinterpret_cast<unsigned long long*>(summary_dev)};
  const int32_t nblk = (int32_t)std::min<int64_t>(((int64_t)n + 3) / 4, CNA_BLOCKS);
  if (summary_dev) hipLaunchKernelGGL(k_cna_zero, dim3(1), dim3(WAVE), 0, s, status, g.summary);
  return dispatch_t_off(h, [&](auto t, auto off) -> int {
    using T = decltype(t);
    using OFF = decltype(off);
    const LjArgs<T, OFF> a = lj_args<T, OFF>(h, q_dev, stride, status);
    with_flag(h->plan.tilt, [&](auto tri) {
      with_flag(mode == NL_CNA_ADAPTIVE, [&](auto ad) {
        hipLaunchKernelGGL((k_cna<T, OFF, decltype(tri)::value, decltype(ad)::value>), dim3(nblk), dim3(STAGE_THREADS), 0, s, a, g);
      });
    });
    HIPCHK(h, hipGetLastError());
    return NL_OK;
  });
}

// Steinhardt's lists (a row must hold every neighbour of its centre: a whole single-device FULL list) and reach (a pair of types
// with rc_ab = 0 is no neighbour pair and asks for nothing).
int cna_reach(nl_handle_t h, double r_max, double skin) {
  if (!h->plan.full || h->args.slab || h->args.gid || h->args.dyn || h->n_rows != h->n) return fail(h, NL_ERR_STATE);
  return r_max <= list_reach(h, /*skip_zero=*/true) - skin ? NL_OK : fail(h, NL_ERR_ARG);
}

int cna_call(nl_handle_t h, const void* q_dev, int32_t q_stride, int mode, double r_max, int32_t* type_dev, int32_t* counts_dev,
             int64_t* summary_dev, void* stream, bool enqueue) {
  return consumer_call(
      h, q_dev, q_stride, type_dev, r_max > 0 && std::isfinite(r_max) && (mode == NL_CNA_FIXED || mode == NL_CNA_ADAPTIVE), stream,
      enqueue, [&](double skin) { return cna_reach(h, r_max, skin); },
      [&](hipStream_t s, const uint32_t* status) {
        return cna_launch(h, q_dev, q_stride, mode, r_max, type_dev, counts_dev, summary_dev, s, status);
      });
}

}  // namespace

extern "C" {

int nl_cna(nl_handle_t h, const void* q_dev, int32_t q_stride, int mode, double r_max, int32_t* type_dev, int32_t* counts_dev,
           int64_t* summary_dev, void* stream) {
  return cna_call(h, q_dev, q_stride, mode, r_max, type_dev, counts_dev, summary_dev, stream, false);
}
int nl_cna_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, int mode, double r_max, int32_t* type_dev, int32_t* counts_dev,
                   int64_t* summary_dev, void* stream) {
  return cna_call(h, q_dev, q_stride, mode, r_max, type_dev, counts_dev, summary_dev, stream, true);
}

}  // extern "C"
