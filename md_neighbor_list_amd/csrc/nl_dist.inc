// nl_dist.inc -- the domain-decomposed build behind the C ABI (SURVEY.md section 8b/8e): nl_comm_create*,
// nl_make_list_distributed.  No reference counterpart: the reference is single GPU (make_list.cu:122-127).
//
// The global mesh (the reference's, int(L / rc) per axis) is cut along z into contiguous runs of cell layers, one rank
// per GPU (the same split as md_neighbor_list_amd/slab.py: as even as possible, the first mz % world ranks one layer
// more).  A steady-state build involves NO host synchronisation (round 3; round 2 waited three times per build):
//   1. k_pack_layers packs the rank's two boundary layers (the owned particles whose cell lies in layer z_lo / z_hi - 1,
//      wave-aggregated appends) into two messages of FIXED capacity, the particle count in a header element in front;
//   2. the four messages of a rank (down, up, from above, from below) travel as one group of ncclSend / ncclRecv over
//      xGMI on a communication stream -- or through a caller-supplied host transport (tests: torch.distributed gloo);
//      their sizes are the capacities, which both ends of a message know, not the counts, which only the sender knows;
//   3. k_unpack_ghosts reads the two received counts on the device, writes the ghosts behind the owned rows
//      q[n_owned ...) of the caller's position buffer and leaves the counts where the build reads them;
//   4. nl_make_list_slab builds rows for the owned particles; how many ghosts there are it learns from device memory
//      (BinPhase::dyn), the host having sized the launches for the capacities.
// Capacities are NEGOTIATED (blocking: the counts are read back and exchanged) in a handle's first build and again after
// a build in which a layer outgrew its message (the build reports NL_ERR_CAPACITY at its synchronisation; a synchronous
// build renegotiates and repeats itself): count + 25 % + 1024, the same formula at both ends of a message.  In a moving
// system the counts change from build to build and nothing is renegotiated until a layer grows by a quarter.
// Stream order replaces the host waits: the pack kernel waits for the previous sends (it overwrites their buffers), the
// receives for the previous unpack (it reads theirs); ghosts are unpacked on the build stream, behind the previous build.
// Positions travel unshifted (no minimum image in the reference: neighlist_cpu.hpp:219-223; nl_set_periodic handles the
// images on the receiving side), global ids in the w component (NL_GID_IN_W).  No collective on the data path.
// Included at the end of nl_api.hip.

#include <dlfcn.h>
#include <rccl/rccl.h>

// Flags of a build's exchange (counts[4]): which of the rank's four messages was too small for its layer -- both ends of a
// message see it (the sender counts more than the capacity, the receiver reads that count in the header), so both
// renegotiate exactly that message before their next build -- and whether the ghosts fit the caller's rows.
enum : int32_t { HALO_SEND_LO = 1, HALO_SEND_HI = 2, HALO_RECV_LO = 4, HALO_RECV_HI = 8, HALO_MESSAGES = 15, HALO_ROWS_OVERFLOW = 16 };

struct nl_comm_s {
  int rank = 0, world = 1, device = 0;
  // RCCL, resolved at run time (dlopen): the library has no link-time dependency on it
  void* lib = nullptr;
  ncclComm_t comm = nullptr;
  ncclResult_t (*p_CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*p_CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*p_Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*p_Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*p_GroupStart)() = nullptr;
  ncclResult_t (*p_GroupEnd)() = nullptr;
  // caller-supplied host transport
  nl_sendrecv_fn fn = nullptr;
  void* user = nullptr;
  // message buffers: [header element | cap particles] each; send: down (my bottom layer), up; recv: from below, from above
  DevBuf<void> send_buf[2];
  DevBuf<void> recv_buf[2];
  int64_t scap[2] = {0, 0}, rcap[2] = {0, 0};  // negotiated capacities (particles) of the four messages
  int64_t salloc[2] = {0, 0}, ralloc[2] = {0, 0};  // particles the buffers have room for
  size_t elem = 0;           // bytes per particle (and of the header element)
  int32_t need = HALO_MESSAGES;    // messages whose capacity has to be (re)negotiated before the next build
  DevBuf<int32_t> counts_dev;      // [0..1] packed counts (bottom, top), [2..3] ghost counts (from below, from above), [4] flags
  int32_t* counts_host = nullptr;  // pinned mirror, copied with every build
  bool check_pending = false;      // an asynchronous build's flags have not been looked at yet
  void* stage_host = nullptr;      // host staging of the callback transport
  size_t stage_bytes = 0;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_ready = nullptr, ev_done = nullptr, ev_sent = nullptr, ev_unpacked = nullptr, ev_result = nullptr;
  int32_t z_lo = 0, z_hi = 0;
  nl_handle_t last_h = nullptr;    // the handle whose builds read counts_host (nl_comm_destroy detaches it)
};

namespace {

void* rccl_open() {
  for (const char* name : {"librccl.so.1", "librccl.so"}) {
    if (void* l = dlopen(name, RTLD_NOW | RTLD_NOLOAD)) return l;  // the copy the process already uses (e.g. PyTorch's)
  }
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    if (void* l = dlopen(name, RTLD_NOW | RTLD_LOCAL)) return l;
  }
  return nullptr;
}

// [z_lo, z_hi) of every rank: contiguous, as even as possible (md_neighbor_list_amd/slab.py split_layers)
bool split_layers(int32_t mz, int world, int rank, int32_t* z_lo, int32_t* z_hi) {
  if (world < 1 || mz < 3 || rank < 0 || rank >= world) return false;
  const int32_t base = mz / world, rem = mz % world;
  if (world > 1 && (base < 1 || mz - (base + (rem ? 1 : 0)) < 2)) return false;  // the two ghost layers must differ
  *z_lo = rank * base + std::min<int32_t>(rank, rem);
  *z_hi = *z_lo + base + (rank < rem ? 1 : 0);
  return true;
}

// The owned particles of the two boundary layers, appended behind the header element of their message: send_lo (layer
// z_lo, at most cap_lo particles) and send_hi (layer z_hi - 1); counts[0], counts[1] = how many there are (may exceed the
// capacity: nothing is written beyond it).  The layer of a particle is the reference's hash (local_cell).
template <typename T>
__global__ void __launch_bounds__(256) k_pack_layers(const T* __restrict__ q, int32_t n_owned, Grid<T> g, T* __restrict__ send_lo,
                                                     T* __restrict__ send_hi, int32_t cap_lo, int32_t cap_hi, int32_t* __restrict__ counts) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool lo = false, hi = false;
  T v[4] = {0, 0, 0, 0};
  if (i < n_owned) {
    const T* p = q + (size_t)i * 4;
    if constexpr (sizeof(T) == 4) {
      const float4 f = *reinterpret_cast<const float4*>(p);
      v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
    } else {
      const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
      v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    }
    int32_t lz = 0;
    const int32_t c = local_cell(g, v[0], v[1], v[2], &lz);
    lo = c >= 0 && lz == 1;
    hi = c >= 0 && lz == g.mzl - 2;
  }
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const bool mine = side ? hi : lo;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
    if (m == 0) continue;  // wave-uniform
    int32_t base = 0;
    if (lane == 0) base = atomicAdd(&counts[side], (int32_t)__popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    const int32_t at = base + (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (mine && at < (side ? cap_hi : cap_lo)) {
      T* d = (side ? send_hi : send_lo) + ((size_t)1 + at) * 4;  // (element 0 is the header)
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        *reinterpret_cast<double2*>(d) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2*>(d + 2) = make_double2(v[2], v[3]);
      }
    }
  }
}

// The headers of the two messages: the counts (as packed; a count beyond the capacity raises HALO_SEND_* here and
// HALO_RECV_* at the receiver, which takes none of that layer).
__global__ void k_pack_headers(int32_t* __restrict__ hdr_lo, int32_t* __restrict__ hdr_hi, int32_t cap_lo, int32_t cap_hi,
                               int32_t* __restrict__ counts) {
  if (threadIdx.x == 0) {
    hdr_lo[0] = counts[0], hdr_hi[0] = counts[1];
    if (counts[0] > cap_lo) atomicOr(&counts[4], HALO_SEND_LO);
    if (counts[1] > cap_hi) atomicOr(&counts[4], HALO_SEND_HI);
  }
}

// The ghosts behind the owned rows: from below (layer z_lo - 1) at q[n_owned ...), from above behind them; counts[2],
// counts[3] = how many (what the build reads through BinPhase::dyn).  A layer that did not fit its message, or ghosts
// that do not fit the rows the caller and the handle have room for, raise a flag and count as none.
template <typename T>
__global__ void __launch_bounds__(256) k_unpack_ghosts(const T* __restrict__ from_lo, const T* __restrict__ from_hi, int32_t cap_lo, int32_t cap_hi,
                                                       T* __restrict__ q, int32_t n_owned, int64_t room, int32_t* __restrict__ counts) {
  int32_t n_lo = reinterpret_cast<const int32_t*>(from_lo)[0], n_hi = reinterpret_cast<const int32_t*>(from_hi)[0];
  int32_t flags = 0;
  if (n_lo < 0 || n_lo > cap_lo) flags |= HALO_RECV_LO, n_lo = 0;
  if (n_hi < 0 || n_hi > cap_hi) flags |= HALO_RECV_HI, n_hi = 0;
  if ((int64_t)n_owned + n_lo + n_hi > room) flags |= HALO_ROWS_OVERFLOW, n_lo = 0, n_hi = 0;
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    counts[2] = n_lo, counts[3] = n_hi;
    if (flags) atomicOr(&counts[4], flags);
  }
  typedef typename std::conditional<sizeof(T) == 4, float4, double4>::type V;
  if (i < n_lo) reinterpret_cast<V*>(q)[(size_t)n_owned + i] = reinterpret_cast<const V*>(from_lo)[1 + i];
  if (i < n_hi) reinterpret_cast<V*>(q)[(size_t)n_owned + n_lo + i] = reinterpret_cast<const V*>(from_hi)[1 + i];
}

int comm_alloc(nl_comm_t c) {
  if (hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking) != hipSuccess) return NL_ERR_HIP;
  for (hipEvent_t* e : {&c->ev_ready, &c->ev_done, &c->ev_sent, &c->ev_unpacked, &c->ev_result})
    if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return NL_ERR_HIP;
  if (c->counts_dev.replace(8 * sizeof(int32_t)) != hipSuccess) return NL_ERR_NOMEM;
  if (hipMemset(c->counts_dev, 0, 8 * sizeof(int32_t)) != hipSuccess) return NL_ERR_HIP;
  if (hipHostMalloc(reinterpret_cast<void**>(&c->counts_host), 8 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) return NL_ERR_NOMEM;
  memset(c->counts_host, 0, 8 * sizeof(int32_t));
  return NL_OK;
}

// message capacity for a layer of `count` particles: the same value at both ends of the message
int64_t halo_capacity(int32_t count) { return (int64_t)count + count / 4 + 1024; }

// room for the four messages at their negotiated capacities (header element + particles)
int comm_grow(nl_comm_t c, size_t elem) {
  if (elem > c->elem) {
    for (int k = 0; k < 2; k++) c->salloc[k] = c->ralloc[k] = 0;  // wider elements: everything anew
    c->elem = elem;
  }
  for (int k = 0; k < 2; k++) {
    if (c->scap[k] > c->salloc[k]) {
      if (c->send_buf[k].replace(((size_t)c->scap[k] + 1) * c->elem + 64) != hipSuccess) return NL_ERR_NOMEM;
      c->salloc[k] = c->scap[k];
    }
    if (c->rcap[k] > c->ralloc[k]) {
      if (c->recv_buf[k].replace(((size_t)c->rcap[k] + 1) * c->elem + 64) != hipSuccess) return NL_ERR_NOMEM;
      c->ralloc[k] = c->rcap[k];
    }
  }
  return NL_OK;
}

// one message each way with the two z-neighbours: send `lo` down and `hi` up, receive from above into from_hi and from
// below into from_lo.  RCCL: device pointers, one group on `s`.  Callbacks: host pointers, blocking.
int comm_exchange(nl_handle_t h, nl_comm_t c, const void* lo, size_t lo_bytes, const void* hi, size_t hi_bytes, void* from_lo,
                  size_t from_lo_bytes, void* from_hi, size_t from_hi_bytes, hipStream_t s) {
  const int lo_peer = (c->rank - 1 + c->world) % c->world, hi_peer = (c->rank + 1) % c->world;
  if (c->comm) {
    // With world == 2 both neighbours are the same rank: its first message (its bottom layer) is MY upper ghost layer,
    // so the receive from above is posted first; messages between two ranks match in posting order.
    if (c->p_GroupStart() != ncclSuccess) return fail(h, NL_ERR_COMM);
    ncclResult_t r = ncclSuccess;
    if (lo_bytes) r = c->p_Send(lo, lo_bytes, ncclChar, lo_peer, c->comm, s);
    if (r == ncclSuccess && hi_bytes) r = c->p_Send(hi, hi_bytes, ncclChar, hi_peer, c->comm, s);
    if (r == ncclSuccess && from_hi_bytes) r = c->p_Recv(from_hi, from_hi_bytes, ncclChar, hi_peer, c->comm, s);
    if (r == ncclSuccess && from_lo_bytes) r = c->p_Recv(from_lo, from_lo_bytes, ncclChar, lo_peer, c->comm, s);
    if (c->p_GroupEnd() != ncclSuccess || r != ncclSuccess) return fail(h, NL_ERR_COMM);
    return NL_OK;
  }
  // host transport: two shifts around the ring (everybody sends down and receives from above, then the other way)
  if (c->fn(c->user, lo_peer, lo, lo_bytes, hi_peer, from_hi, from_hi_bytes) != 0) return fail(h, NL_ERR_COMM);
  if (c->fn(c->user, hi_peer, hi, hi_bytes, lo_peer, from_lo, from_lo_bytes) != 0) return fail(h, NL_ERR_COMM);
  return NL_OK;
}

}  // namespace

extern "C" {

int nl_comm_unique_id(void* id_out) {
  if (!id_out) return NL_ERR_ARG;
  void* lib = rccl_open();
  if (!lib) return NL_ERR_COMM;
  auto get = reinterpret_cast<ncclResult_t (*)(ncclUniqueId*)>(dlsym(lib, "ncclGetUniqueId"));
  if (!get) return NL_ERR_COMM;
  ncclUniqueId id;
  if (get(&id) != ncclSuccess) return NL_ERR_COMM;
  memcpy(id_out, &id, sizeof(id));
  return NL_OK;
}

int nl_comm_destroy(nl_comm_t c) {
  if (!c) return NL_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
  if (c->comm && c->p_CommDestroy) (void)c->p_CommDestroy(c->comm);
  if (c->last_h && c->last_h->args.dyn_host == c->counts_host) c->last_h->args.dyn_host = nullptr, c->last_h->args.dyn = nullptr;
  if (c->counts_host) (void)hipHostFree(c->counts_host);
  if (c->stage_host) (void)hipHostFree(c->stage_host);
  for (hipEvent_t e : {c->ev_ready, c->ev_done, c->ev_sent, c->ev_unpacked, c->ev_result})
    if (e) (void)hipEventDestroy(e);
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  delete c;  // (the message buffers and counts_dev: each DevBuf frees its own)
  return NL_OK;
}

int nl_comm_create(nl_comm_t* out, int rank, int world, const void* unique_id, int device_id) {
  if (!out) return NL_ERR_ARG;
  *out = nullptr;
  if (world < 1 || rank < 0 || rank >= world || !unique_id) return NL_ERR_ARG;
  int dev = device_id;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return NL_ERR_NO_DEVICE;
  if (hipSetDevice(dev) != hipSuccess) return NL_ERR_NO_DEVICE;
  nl_comm_t c = new (std::nothrow) nl_comm_s();
  if (!c) return NL_ERR_NOMEM;
  c->rank = rank, c->world = world, c->device = dev;
  c->lib = rccl_open();
  if (c->lib) {
    c->p_CommInitRank = reinterpret_cast<decltype(c->p_CommInitRank)>(dlsym(c->lib, "ncclCommInitRank"));
    c->p_CommDestroy = reinterpret_cast<decltype(c->p_CommDestroy)>(dlsym(c->lib, "ncclCommDestroy"));
    c->p_Send = reinterpret_cast<decltype(c->p_Send)>(dlsym(c->lib, "ncclSend"));
    c->p_Recv = reinterpret_cast<decltype(c->p_Recv)>(dlsym(c->lib, "ncclRecv"));
    c->p_GroupStart = reinterpret_cast<decltype(c->p_GroupStart)>(dlsym(c->lib, "ncclGroupStart"));
    c->p_GroupEnd = reinterpret_cast<decltype(c->p_GroupEnd)>(dlsym(c->lib, "ncclGroupEnd"));
  }
  if (!c->p_CommInitRank || !c->p_CommDestroy || !c->p_Send || !c->p_Recv || !c->p_GroupStart || !c->p_GroupEnd) {
    nl_comm_destroy(c);
    return NL_ERR_COMM;
  }
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  if (c->p_CommInitRank(&c->comm, world, id, rank) != ncclSuccess) {
    c->comm = nullptr;
    nl_comm_destroy(c);
    return NL_ERR_COMM;
  }
  if (int rc = comm_alloc(c)) {
    nl_comm_destroy(c);
    return rc;
  }
  *out = c;
  return NL_OK;
}

int nl_comm_create_callbacks(nl_comm_t* out, int rank, int world, nl_sendrecv_fn fn, void* user, int device_id) {
  if (!out) return NL_ERR_ARG;
  *out = nullptr;
  if (world < 1 || rank < 0 || rank >= world || (!fn && world > 1)) return NL_ERR_ARG;
  int dev = device_id;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return NL_ERR_NO_DEVICE;
  if (hipSetDevice(dev) != hipSuccess) return NL_ERR_NO_DEVICE;
  nl_comm_t c = new (std::nothrow) nl_comm_s();
  if (!c) return NL_ERR_NOMEM;
  c->rank = rank, c->world = world, c->device = dev, c->fn = fn, c->user = user;
  if (int rc = comm_alloc(c)) {
    nl_comm_destroy(c);
    return rc;
  }
  *out = c;
  return NL_OK;
}

int nl_comm_layers(nl_handle_t h, nl_comm_t c, int32_t* z_lo, int32_t* z_hi) {
  if (!h || !c) return NL_ERR_ARG;
  int32_t lo = 0, hi = 0;
  if (!split_layers(h->m[2], c->world, c->rank, &lo, &hi)) return fail(h, NL_ERR_ARG);
  if (z_lo) *z_lo = lo;
  if (z_hi) *z_hi = hi;
  return NL_OK;
}

int nl_distributed_ghosts(nl_comm_t c, int32_t* n_ghost_lo, int32_t* n_ghost_hi) {
  if (!c) return NL_ERR_ARG;
  if (c->last_h) {  // the counts arrive with the build's result
    const int rc = nl_synchronize(c->last_h);
    if (rc && rc != NL_ERR_CAPACITY) return rc;
  }
  if (n_ghost_lo) *n_ghost_lo = c->world > 1 ? c->counts_host[2] : 0;
  if (n_ghost_hi) *n_ghost_hi = c->world > 1 ? c->counts_host[3] : 0;
  return NL_OK;
}

}  // extern "C"

namespace {

template <typename T> void launch_pack(nl_handle_t h, nl_comm_t c, const void* q_dev, int32_t n_owned, int32_t z_lo, int32_t mzl, int32_t cap_lo,
                                       int32_t cap_hi, hipStream_t s) {
  if (n_owned <= 0) return;
  BuildArgs a;  // (the owned rows of a slab build)
  a.n_rows = n_owned, a.z_lo = z_lo, a.mzl = mzl, a.slab = 1;
  hipLaunchKernelGGL(k_pack_layers<T>, dim3((n_owned + 255) / 256), dim3(256), 0, s, static_cast<const T*>(q_dev), n_owned,
                     make_grid<T>(h, a, h->pbc), static_cast<T*>(c->send_buf[0]), static_cast<T*>(c->send_buf[1]), cap_lo, cap_hi,
                     c->counts_dev);
}

// Blocking: (re)negotiates the capacities of the messages in c->need.  The sender of a message counts its layer and tells
// the receiver; both set the capacity from that count.  (The first build of a communicator negotiates all four.)
int negotiate(nl_handle_t h, nl_comm_t c, const void* q_dev, int32_t n_owned, int32_t z_lo, int32_t mzl, size_t elem, hipStream_t s) {
  int32_t* cnt = c->counts_host;
  const int32_t need = c->need;
  HIPCHK(h, hipStreamSynchronize(s));  // (whatever the previous build still sends or unpacks)
  HIPCHK(h, hipStreamSynchronize(c->comm_stream));
  HIPCHK(h, hipMemsetAsync(c->counts_dev, 0, 8 * sizeof(int32_t), s));
  if (h->dtype == NL_F32) launch_pack<float>(h, c, q_dev, n_owned, z_lo, mzl, 0, 0, s);  // capacity 0: counts only
  else launch_pack<double>(h, c, q_dev, n_owned, z_lo, mzl, 0, 0, s);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(cnt, c->counts_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  // my bottom count goes down (it is the lower rank's count from above), my top count goes up
  const size_t s_lo = need & HALO_SEND_LO ? 4 : 0, s_hi = need & HALO_SEND_HI ? 4 : 0, r_lo = need & HALO_RECV_LO ? 4 : 0, r_hi = need & HALO_RECV_HI ? 4 : 0;
  if (c->comm) {
    if (int rc = comm_exchange(h, c, c->counts_dev, s_lo, c->counts_dev + 1, s_hi, c->counts_dev + 2, r_lo, c->counts_dev + 3, r_hi, s)) return rc;
    HIPCHK(h, hipMemcpyAsync(cnt + 2, c->counts_dev + 2, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
  } else {
    if (int rc = comm_exchange(h, c, cnt, s_lo, cnt + 1, s_hi, cnt + 2, r_lo, cnt + 3, r_hi, s)) return rc;
  }
  if ((r_lo && cnt[2] < 0) || (r_hi && cnt[3] < 0)) return fail(h, NL_ERR_COMM);
  if (s_lo) c->scap[0] = halo_capacity(cnt[0]);
  if (s_hi) c->scap[1] = halo_capacity(cnt[1]);
  if (r_lo) c->rcap[0] = halo_capacity(cnt[2]);
  if (r_hi) c->rcap[1] = halo_capacity(cnt[3]);
  if (int rc = comm_grow(c, elem)) return fail(h, rc);
  c->need = 0;
  return NL_OK;
}

}  // namespace

extern "C" {

int nl_make_list_distributed(nl_handle_t h, nl_comm_t c, void* q_dev, int32_t q_capacity, int32_t n_owned, void* stream, int sync) {
  if (!h || !c) return NL_ERR_ARG;
  if (h->local_ids) return fail(h, NL_ERR_STATE);  // (nl_set_local_ids: these lists hold global ids, their ghost counts live on the device)
  if (filter_rows_only(h)) return fail(h, NL_ERR_STATE);  // (nl_set_exclusions, nl_set_type_cutoffs: whole single-device builds only)
  if (box_changed(h)) return fail(h, NL_ERR_STATE);    // (nl_set_box: the layers are those of nl_create's box)
  if (h->pair_images) return fail(h, NL_ERR_STATE);    // (nl_set_pair_images: whole single-device builds only)
  if (n_owned < 0 || q_capacity < n_owned || (!q_dev && q_capacity > 0)) return fail(h, NL_ERR_ARG);
  if (c->device != h->device) return fail(h, NL_ERR_ARG);
  int32_t z_lo = 0, z_hi = 0;
  if (!split_layers(h->m[2], c->world, c->rank, &z_lo, &z_hi)) return fail(h, NL_ERR_ARG);
  c->z_lo = z_lo, c->z_hi = z_hi;
  if (c->last_h && c->last_h != h && c->last_h->args.dyn_host == c->counts_host)
    c->last_h->args.dyn_host = nullptr, c->last_h->args.dyn = nullptr;
  c->last_h = h;
  if (c->world == 1) {  // the whole box: the periodic wrap stays inside the build
    return nl_make_list_slab(h, q_dev, 4, NL_GID_IN_W, n_owned, n_owned, 0, h->m[2], stream, sync);
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t elem = h->dtype == NL_F32 ? 16 : 32;
  const int32_t mzl = (z_hi - z_lo) + 2;
  int32_t* cnt = c->counts_host;
  // the device-side ghost counts need the two-level binning (BinPhase::dyn); meshes beyond its tables take the atomic-rank
  // path, which wants the particle count on the host: there the counts are read back (one wait per build)
  const bool dyn_ok = two_level_ok(h, mzl);
  // an earlier asynchronous build whose result has arrived: did its messages hold what was sent?
  if (c->check_pending && hipEventQuery(c->ev_result) == hipSuccess) {
    c->check_pending = false;
    c->need |= cnt[4] & HALO_MESSAGES;
  }
  for (int attempt = 0;; attempt++) {
    if (h->pending && h->last_stream != s) {  // (the previous build ran on another stream)
      HIPCHK(h, hipStreamSynchronize(h->last_stream));
      h->pending = false;
    }
    if (elem != c->elem) c->need = HALO_MESSAGES;
    if (c->need)
      if (int rc = negotiate(h, c, q_dev, n_owned, z_lo, mzl, elem, s)) return rc;
    const int32_t cap_lo = (int32_t)c->scap[0], cap_hi = (int32_t)c->scap[1], rcap_lo = (int32_t)c->rcap[0], rcap_hi = (int32_t)c->rcap[1];
    const int64_t room = std::min<int64_t>(q_capacity, h->n_max);
    // ---- pack (behind the previous sends: it overwrites their buffers)
    if (c->comm) HIPCHK(h, hipStreamWaitEvent(s, c->ev_sent, 0));
    HIPCHK(h, hipMemsetAsync(c->counts_dev, 0, 8 * sizeof(int32_t), s));
    if (h->dtype == NL_F32) launch_pack<float>(h, c, q_dev, n_owned, z_lo, mzl, cap_lo, cap_hi, s);
    else launch_pack<double>(h, c, q_dev, n_owned, z_lo, mzl, cap_lo, cap_hi, s);
    hipLaunchKernelGGL(k_pack_headers, dim3(1), dim3(64), 0, s, static_cast<int32_t*>(c->send_buf[0]), static_cast<int32_t*>(c->send_buf[1]),
                       cap_lo, cap_hi, c->counts_dev);
    HIPCHK(h, hipGetLastError());
    const size_t b_lo = ((size_t)cap_lo + 1) * elem, b_hi = ((size_t)cap_hi + 1) * elem;
    const size_t r_lo = ((size_t)rcap_lo + 1) * elem, r_hi = ((size_t)rcap_hi + 1) * elem;
    // ---- the four messages, sized by their capacities
    if (c->comm) {
      HIPCHK(h, hipEventRecord(c->ev_ready, s));
      HIPCHK(h, hipStreamWaitEvent(c->comm_stream, c->ev_ready, 0));
      HIPCHK(h, hipStreamWaitEvent(c->comm_stream, c->ev_unpacked, 0));  // the previous unpack has read the receive buffers
      if (int rc = comm_exchange(h, c, c->send_buf[0], b_lo, c->send_buf[1], b_hi, c->recv_buf[0], r_lo, c->recv_buf[1], r_hi, c->comm_stream))
        return rc;
      HIPCHK(h, hipEventRecord(c->ev_sent, c->comm_stream));
      HIPCHK(h, hipEventRecord(c->ev_done, c->comm_stream));
      HIPCHK(h, hipStreamWaitEvent(s, c->ev_done, 0));
    } else {  // host transport (blocking by nature): staged through pinned memory
      const size_t need = b_lo + b_hi + r_lo + r_hi + 64;
      if (need > c->stage_bytes) {
        if (c->stage_host) (void)hipHostFree(c->stage_host);
        c->stage_host = nullptr, c->stage_bytes = 0;
        if (hipHostMalloc(&c->stage_host, need + need / 4, hipHostMallocDefault) != hipSuccess) return fail(h, NL_ERR_NOMEM);
        c->stage_bytes = need + need / 4;
      }
      char* const st_lo = static_cast<char*>(c->stage_host);
      char* const st_hi = st_lo + b_lo;
      char* const st_from_lo = st_hi + b_hi;
      char* const st_from_hi = st_from_lo + r_lo;
      HIPCHK(h, hipMemcpyAsync(st_lo, c->send_buf[0], b_lo, hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipMemcpyAsync(st_hi, c->send_buf[1], b_hi, hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      if (int rc = comm_exchange(h, c, st_lo, b_lo, st_hi, b_hi, st_from_lo, r_lo, st_from_hi, r_hi, s)) return rc;
      HIPCHK(h, hipMemcpyAsync(c->recv_buf[0], st_from_lo, r_lo, hipMemcpyHostToDevice, s));
      HIPCHK(h, hipMemcpyAsync(c->recv_buf[1], st_from_hi, r_hi, hipMemcpyHostToDevice, s));
    }
    // ---- ghosts behind the owned rows, their counts into counts_dev[2..3]
    {
      const int32_t most = std::max(rcap_lo, rcap_hi);
      if (h->dtype == NL_F32)
        hipLaunchKernelGGL(k_unpack_ghosts<float>, dim3((most + 255) / 256), dim3(256), 0, s, static_cast<const float*>(c->recv_buf[0]),
                           static_cast<const float*>(c->recv_buf[1]), rcap_lo, rcap_hi, static_cast<float*>(q_dev), n_owned, room, c->counts_dev);
      else
        hipLaunchKernelGGL(k_unpack_ghosts<double>, dim3((most + 255) / 256), dim3(256), 0, s, static_cast<const double*>(c->recv_buf[0]),
                           static_cast<const double*>(c->recv_buf[1]), rcap_lo, rcap_hi, static_cast<double*>(q_dev), n_owned, room, c->counts_dev);
      HIPCHK(h, hipGetLastError());
      if (c->comm) HIPCHK(h, hipEventRecord(c->ev_unpacked, s));
    }
    HIPCHK(h, hipMemcpyAsync(cnt, c->counts_dev, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipEventRecord(c->ev_result, s));
    int rc;
    if (dyn_ok) {
      // the build: as many rows as the messages can bring at most; how many ghosts there are it reads on the device
      const int32_t n_upper = (int32_t)std::min<int64_t>((int64_t)n_owned + rcap_lo + rcap_hi, room);
      BuildArgs a{q_dev, 4, NL_GID_IN_W, n_owned, n_upper, 0, z_lo};
      a.dyn = c->counts_dev + 2, a.dyn_host = cnt;
      a.n_est = (int32_t)std::min<int64_t>(n_upper, (int64_t)n_owned + (c->rcap[0] - 1024) * 4 / 5 + (c->rcap[1] - 1024) * 4 / 5);
      rc = make_list_slab_part(h, a, z_hi, stream, sync, PART_ALL);
    } else {
      HIPCHK(h, hipStreamSynchronize(s));
      rc = cnt[4] ? NL_ERR_CAPACITY : nl_make_list_slab(h, q_dev, 4, NL_GID_IN_W, n_owned, n_owned + cnt[2] + cnt[3], z_lo, z_hi, stream, sync);
    }
    const bool finished = sync || !dyn_ok;  // cnt[] is this build's
    if (finished && cnt[4]) {
      if (cnt[4] & HALO_ROWS_OVERFLOW) return fail(h, NL_ERR_CAPACITY);  // (the caller's rows are too few: no capacity of ours helps)
      c->need |= cnt[4] & HALO_MESSAGES;  // a layer outgrew its message: a new capacity for it, and the build once more
      if (attempt == 0) continue;
      return fail(h, NL_ERR_CAPACITY);
    }
    if (!finished) c->check_pending = true;
    return rc;
  }
}

}  // extern "C"
