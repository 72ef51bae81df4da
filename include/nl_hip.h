/*
 * nl_hip.h -- C ABI of libnl_hip.so: the MI355X (gfx950) Verlet neighbour-list builder.
 *
 * This is the drop-in boundary for the ONE hot path of kohnakagawa/md_neighbor_list:
 *   cell hash -> sort by cell -> 27-cell pair search with cut-off test -> compaction into the pair list.
 * The reference has no FFI layer; its boundary is the C++ class surface its two harnesses touch
 * (SURVEY.md section 8b).  Every entry point below names the reference interface it replaces
 * (file:line in the reference tree).  The header-only C++ shims include/neighlist_gpu.hpp (GPU harness
 * surface: cuda_ptr<T>, NeighListGPU<Vec,Dtype>) and include/neighlist_cpu.hpp (CPU harness surface:
 * NeighList<Vec>) are built on nothing but these functions.
 *
 * Conventions
 *   - plain C types only; every function returns an nl_status (0 = NL_OK) and never aborts or throws
 *     (the reference aborts through checkCudaErrors / std::exit(1), device_util.cuh:41-54).
 *   - a handle owns every device buffer it hands out; returned device pointers stay valid until the next
 *     nl_make_list* / nl_initialize / nl_destroy on that handle (the reference's accessors return references to
 *     members, neighlist_gpu.hpp:468-482).  The caller owns the position buffer.
 *   - one handle per device per host thread; no global state (the reference keeps function-local statics,
 *     neighlist_gpu.hpp:303, kernel_impl.cuh:222-226, and is not re-entrant).
 *   - the result contract is the reference's SCALAR CPU class (neighlist_cpu.hpp): the half list
 *     {(i,j): i<j, r2 <= rc2} with r2 = (dx*dx + dy*dy) + dz*dz evaluated without FMA in the position type and
 *     compared against a double rc2 (neighlist_cpu.hpp:215-223), over the cell pairs that class visits.
 */
#ifndef NL_HIP_H
#define NL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nl_handle_s* nl_handle_t;

typedef enum nl_dtype {
  NL_F32 = 0, /* Vec = float4-like  {x,y,z,w}, 16 B (make_list.cu:10-11) */
  NL_F64 = 1  /* Vec = double4-like {x,y,z,w}, 32 B (make_list.cu:7-8)   */
} nl_dtype;

typedef enum nl_status {
  NL_OK = 0,
  NL_ERR_ARG = 1,            /* null/negative/inconsistent argument                                            */
  NL_ERR_NOMEM = 2,          /* host or device allocation failed                                               */
  NL_ERR_OUT_OF_BOX = 3,     /* a coordinate is NaN or more than one box length outside [0,L): the reference
                                indexes out of bounds there (GenHash + one ApplyPBC wrap, neighlist_cpu.hpp:51-66) */
  NL_ERR_CAPACITY = 4,       /* pair list larger than the capacity set for this handle (async builds only;
                                the reference silently overruns MAX_PARTNERS*N, neighlist_cpu.hpp:37,76-78)    */
  NL_ERR_HIP = 5,            /* a HIP runtime call failed; see nl_last_hip_error                               */
  NL_ERR_STATE = 6,          /* call order violated (e.g. make_list before initialize, getter before a build)  */
  NL_ERR_MESH = 7,           /* fewer than 3 cells along an axis: the reference visits cell pairs twice there
                                and emits duplicate pairs; this library refuses such boxes                     */
  NL_ERR_INDEX_OVERFLOW = 8, /* the list has more than INT32_MAX entries and a 32-bit key_pointer was asked for:
                                nl_get_*_csr / the transposed list after a wide build, or a build with
                                nl_set_offset_width(32); the reference wraps silently there (neighlist_cpu.hpp:15,29) */
  NL_ERR_NO_DEVICE = 9,      /* no usable gfx950 device / wrong code object                                    */
  NL_ERR_DOMAIN = 10,        /* slab builds: a row particle outside the owned cells or a ghost inside them     */
  NL_ERR_COMM = 11           /* distributed builds: RCCL not loadable / a communicator call or the transport failed */
} nl_status;

const char* nl_status_string(int status);

/* ------------------------------------------------------------------------------------------------ lifecycle */

/* Replaces the constructors NeighListGPU(rc,Lx,Ly,Lz) (neighlist_gpu.hpp:236-255) and NeighList(rc,Lx,Ly,Lz)
 * (neighlist_cpu.hpp:380-395): mesh_size[d] = (int)(L_d / rc), ms = L/mesh_size, rc2 = rc*rc in double; ms and
 * 1/ms are rounded to `dtype` exactly as the CPU class stores them in a Vec (neighlist_cpu.hpp:12,389-391,409-411).
 * device_id < 0 selects the current HIP device. */
int nl_create(nl_handle_t* out, int dtype, double rc, double Lx, double Ly, double Lz, int device_id);

/* Replaces Initialize(N) (neighlist_gpu.hpp:268-287, neighlist_cpu.hpp:408-415): allocates every per-particle and
 * per-cell buffer for up to n_max particles.  The pair-list capacity defaults to an estimate from the number
 * density (1.3 x the ideal-gas half count + slack); see nl_set_capacity. Call once, or again to grow.  A second call
 * drops the list and every buffer sized by the old n_max (the transposed list among them); exclusion and type tables
 * are kept: they go on filtering builds of their own n and refuse others (NL_ERR_ARG) until they are set again. */
int nl_initialize(nl_handle_t h, int32_t n_max);

/* Pair-list capacity in entries (int32 each).  A synchronous build grows the list by itself; an asynchronous
 * one (sync = 0) cannot, and reports NL_ERR_CAPACITY at the next synchronising call instead of overrunning. */
int nl_set_capacity(nl_handle_t h, int64_t max_pairs);

/* Which list the builds of this handle produce.  NL_LIST_HALF (default): the scalar CPU class's contract, every
 * pair once, in the row of min(i, j) (neighlist_cpu.hpp:233-236).  NL_LIST_FULL: the GPU kernels' contract, every
 * pair in both rows (kernel_impl.cuh:24-33: every j != i within the cut-off), as a CSR in original particle order;
 * nl_get_full_transposed then turns it into the GPU class's list[k*N + i] with coalesced writes instead of
 * deriving it from the half list.  Takes effect at the next build; the list capacity is counted in entries
 * (a full list has twice as many) and is re-estimated unless it was set by nl_set_capacity. */
enum nl_list_kind { NL_LIST_HALF = 0, NL_LIST_FULL = 1 };
int nl_set_list_kind(nl_handle_t h, int kind);

/* Width of the list offsets (key_pointer).  The reference's key_pointer_ and number_of_pairs_ are int32
 * (neighlist_cpu.hpp:15,29; neighlist_gpu.hpp:484-487) and wrap beyond INT32_MAX pairs; BASELINE config 4 has 2.5e9.
 * 0 (default): a build uses 64-bit offsets as soon as the list capacity of the handle exceeds INT32_MAX entries -- which
 * the default capacity estimate does for such boxes, and which a synchronous build that overflows reaches by growing
 * the list -- and 32-bit offsets otherwise; 32 / 64 force one width (a 32-bit build of a longer list fails with
 * NL_ERR_INDEX_OVERFLOW).  Whatever the build used, nl_get_*_csr returns int32 offsets (converted once per build if
 * needed, NL_ERR_INDEX_OVERFLOW if they cannot hold the list) and nl_get_*_csr64 int64 offsets.  NL_OFFSET_WIDTH in
 * the environment sets the default. */
int nl_set_offset_width(nl_handle_t h, int bits);

/* Launch mode of asynchronous builds ("capture launch-bound inner loops in hipGraphs").  on != 0:
 * a build is captured once into a hipGraph (memset, the kernels, the 80-byte result copy) and replayed on the caller's
 * stream by later builds with the same arguments; any change of an argument, of the list kind / periodic mode or of a
 * buffer (growth, nl_initialize) captures again.  Pays on small systems, where a build is ~11 dependent launches
 * (N = 4096: see DESIGN.md); off by default.  Also NL_GRAPH=1 in the environment. */
int nl_set_graph(nl_handle_t h, int on);

/* Distances across the periodic faces.  0 (default) = the reference: the 27-cell stencil wraps cell indices but the
 * distance is taken between the coordinates as given (neighlist_cpu.hpp:107-132,219-223), i.e. an open box.
 * 1 = minimum image (not in the reference): a stencil cell reached through a periodic face
 * is tested at its image, dx = (x_j -+ L) - x_i with the shifted coordinate rounded to the position type first; a
 * particle whose cell index was wrapped (coordinate outside [0, L), or rounding up to the box edge) is itself taken
 * at its image next to that cell.  The pair is decided once, by the row that stores it (the smaller id); with
 * NL_LIST_FULL both rows decide on their own and may differ for a pair within one ulp of the cut-off across a face.
 * Slab builds: the two ghost layers of the box-end ranks are the periodic images (the caller sends the layers
 * unshifted, as for the open box), rounded as a whole build rounds them: a ghost whose own cell index was wrapped is
 * taken at rn(rn(z -+ L) +- L), not at z.  Takes effect at the next build.
 * nl_set_periodic(h, m) is nl_set_periodic_axes(h, m ? 7 : 0). */
int nl_set_periodic(nl_handle_t h, int minimum_image);

/* The minimum image on chosen axes only (a film or an interface: periodic in x and y, open in z).  mask: bit 0 = x,
 * bit 1 = y, bit 2 = z; 0 = the open box (default), 7 = nl_set_periodic(1); outside 0..7 is NL_ERR_ARG.
 *   On an axis in the mask: a stencil cell reached through that axis's face is tested at its image (coordinate -+ L,
 *   rounded to the position type first), and a particle whose cell index was wrapped on that axis is itself stored at
 *   its image, its cell index taken as the floor of q * ims.
 *   On an axis not in the mask neither happens: the coordinate is used as given and the cell index is the reference's
 *   truncation plus one wrap.  The stencil still wraps, so a particle slightly outside [0, L) on an open axis still
 *   finds its neighbours; a pair across an open face is as far apart as its raw coordinates say.
 * Any mask but 0 runs the minimum-image kernels (the cost of mask 7).  Every axis still needs 3 cells (NL_ERR_MESH).
 * Slab builds: the box-end ranks' ghost layers are z-images only with bit 2 set.  With z open they are taken as given
 * and hold partners only of particles whose z lies outside [0, L) (filed into the wrapped layer); where every z lies
 * in [0, L) the caller may send them empty.  The layer that owns a particle is its z cell index by the rule above: with
 * bit 2 set the floor, so a particle at z = -0.3 cells belongs to the top layer's rank, with z open the truncation, which
 * files it into layer 0 (NL_ERR_DOMAIN tells a caller who filed it otherwise).  Side effects as nl_set_periodic: a pending
 * build is finished, the next nl_update_list builds, and a changed mask drops the list.  Takes effect at the next
 * build; nl_get_periodic_axes returns the mask that the next build will use. */
int nl_set_periodic_axes(nl_handle_t h, int mask);
int nl_get_periodic_axes(nl_handle_t h, int* mask);

/* Triclinic boxes and box changes between builds (no reference counterpart: its box is orthogonal and fixed).
 *   Box: LAMMPS convention, origin at 0: a = (Lx, 0, 0), b = (xy, Ly, 0), c = (xz, yz, Lz); a particle belongs to the cell
 *     {la a + lb b + lc c : l in [0, 1)^3}.  nl_create(..., Lx, Ly, Lz, ...) is this box with zero tilt.
 *   Mesh (double): the perpendicular widths w_x = Lx / sqrt(1 + (xy/Ly)^2 + ((xy yz - Ly xz)/(Ly Lz))^2),
 *     w_y = Ly / sqrt(1 + (yz/Lz)^2), w_z = Lz; m_d = (int)(w_d / rc) >= 3 (NL_ERR_MESH); ms_d = L_d / m_d and ims_d rounded
 *     as nl_create rounds them (zero tilt: the mesh, ms and ims of nl_create, bit for bit).  With m_d >= 3 every nonzero
 *     lattice vector is at least 3 rc long: a pair has at most one image within rc, and the 27-cell stencil over cells in
 *     sheared coordinates finds it.
 *   Binning (position type T, round to nearest, no FMA): k_xy = (T)(xy/Ly), k_yz = (T)(yz/Lz),
 *     k_xz = (T)((xz Ly - xy yz)/(Ly Lz)), each a double expression rounded once; x' = (x - y k_xy) - z k_xz,
 *     y' = y - z k_yz, z' = z; the cell index of axis d is the nl_set_periodic_axes rule applied to d' ims_d (floor on a
 *     periodic axis, truncation plus one wrap on an open one, NL_ERR_OUT_OF_BOX beyond one box length).  The wraps
 *     n_d in {-1, 0, +1} of the periodic axes put the particle at its image q + S(n), S(n) = n_a a + n_b b + n_c c in double,
 *     rounded to T once per component and added with one rounding per component (components where S is 0 untouched).
 *     Cell and image are decided once, from the input coordinate.
 *   Search: a stencil segment reached through the faces w = (wx, wy, wz) is staged at q_stored + S(w), rounded the same way;
 *     r2 and the cut-off test are unchanged.  Zero tilt: S(w) = -+(T)L_d, today's lists bit for bit.
 *   A tilt needs periodic axes: xy != 0 needs x and y in the nl_set_periodic_axes mask, xz x and z, yz y and z (the
 *     hexagonal slab, mask 3 with xy only, is allowed).  The setters may come in either order: a build or update that
 *     violates this is NL_ERR_STATE.  Open axes therefore keep the rule of nl_set_periodic_axes exactly.
 *   Skin check (nl_update_list reason (c), double, no FMA): fold the periodic axes z, y, x (LAMMPS' minimum_image order):
 *     k = rint(dz/Lz), dz -= k Lz, dy -= k yz, dx -= k xz; k = rint(dy/Ly), dy -= k Ly, dx -= k xy; dx -= Lx rint(dx/Lx).
 *   nl_lj_forces(_typed)(_enqueue): with a tilt the pair is folded in T in the same order (rint form); every component of
 *     the image within rc is below L_d / 2, so this is the image the list used.  The type filter's r2 is taken at S(w).
 *   nl_set_box: synchronous, finishes a pending build.  A changed box drops the list, makes the next nl_update_list build
 *     (its reason (a)) and captures graphs again; the same box again changes nothing.  Non-finite values or L <= 0 are
 *     NL_ERR_ARG, a mesh of more than 2e9 cells NL_ERR_ARG, any m_d < 3 NL_ERR_MESH, failed growth NL_ERR_NOMEM: an error
 *     leaves the old box, buffers and list.  An initialised handle regrows its per-cell and per-row buffers where the new mesh
 *     needs more; the list capacity is re-estimated from the new volume unless nl_set_capacity set it; exclusion and type
 *     tables are kept; nl_get_mesh reports the mesh of the next build.  Slab and distributed builds are NL_ERR_STATE while
 *     the box differs from nl_create's.
 *   nl_get_box: box = {Lx, Ly, Lz, xy, xz, yz} of the next build. */
int nl_set_box(nl_handle_t h, double Lx, double Ly, double Lz, double xy, double xz, double yz);
int nl_get_box(nl_handle_t h, double box[6]);

int nl_destroy(nl_handle_t h);

/* --------------------------------------------------------------------------------------------------- build */

/* Replaces MakeNeighList(q, N, sync, tblock_size, smem_hei) (neighlist_gpu.hpp:289-466) and MakeNeighList(q, N)
 * (neighlist_cpu.hpp:417-435).  q_dev: device pointer to n positions, `q_stride` scalars apart (4 for the
 * float4/double4 Vec of make_list.cu, 3 for the {x,y,z} Vec of make_list.cpp:26-32).  Positions are read, never
 * reordered (the reference's SortPtclData is commented out, neighlist_cpu.hpp:421).  stream: the hipStream_t the
 * build is enqueued on; NULL is HIP's null (default) stream, where the reference launches (make_list.cu:124-127).
 * The build is ordered after everything already queued on that stream (the kernel that produced q, a halo
 * exchange) and nothing else: positions written on ANOTHER stream must be fenced by the caller.  sync != 0 waits for the build and returns its status; sync == 0 only
 * enqueues (the reference's timing loop, make_list.cu:124-127) and errors surface at the next nl_synchronize /
 * getter.  tblock_size and smem_hei of the reference select among its CUDA variants and have no counterpart.
 * A pending build on another stream is waited for on the host before the new one is enqueued.
 * Tested on a caller's non-blocking stream that a delay holds back, the positions written behind the delay (whatever the
 * build issued on the null stream would read a decoy: the harness checks for every stream it holds that the null stream
 * runs meanwhile; the handle's private stream or an earlier build's stream runs ahead only where the runtime gives it
 * another hardware queue, which is not checked), on every search path, both waits, a grown list, a build that runs
 * again and a second build on another stream; sync == 0 on a handle that has built before returns while the stream is
 * still held: tests/test_caller_stream.py.
 * Tested against the oracle at the mesh sizes where the build changes its binning, its row tables are full and its
 * scans take more than 64 blocks (needles, plates, dilute cubes): tests/test_mesh_limits.py.
 * The cut-off decision itself is pinned down at the last bit -- pairs at rc (1 +- k ulp) in cell corners, on the fine rows'
 * quarter-planes, across every face, a box length outside and in crowded cells -- on every search path, binning, mask,
 * list kind and as slabs: tests/test_cutoff_paths.py. */
int nl_make_list(nl_handle_t h, const void* q_dev, int32_t q_stride, int32_t n, void* stream, int sync);

/* Slab (domain-decomposed) build, SURVEY.md section 8e -- no reference counterpart (the reference is single GPU).
 * The handle describes the GLOBAL box.  This rank owns the cell layers z in [z_lo, z_hi) of the global mesh and
 * passes n_rows owned particles first, then n - n_rows ghost particles lying in the two periodic neighbour layers
 * (z_lo-1 and z_hi, modulo mesh_z).  gid_dev: global particle ids (NULL = identity; NL_GID_IN_W = the id is stored
 * in the w component of each position, as the bit pattern of an int32 (F32) / int64 (F64), which halves the
 * number of halo messages).  Rows are built for the
 * owned particles only: row r holds the global ids j > gid[r] within the cut-off, so that the union over ranks
 * is exactly the global half list.  z_lo = 0, z_hi = mesh_z, n_rows = n is the single-GPU build.
 * After nl_set_list_kind(NL_LIST_FULL): row r holds every global id other than gid[r] within the cut-off, ghosts
 * included, so that the rows over all ranks are exactly the global full list (with a periodic mask each row decides in
 * its own frame, as in a whole build).  Read it with nl_get_full_csr(64), nl_list_checksum and nl_number_of_pairs
 * (entries / 2); nl_get_full_transposed indexes its rows by id and refuses a slab build, half or full (NL_ERR_STATE).
 * Tested row by row against the global list on every search path: tests/test_slab_paths.py. */
#define NL_GID_IN_W ((const int32_t*)1)
int nl_make_list_slab(nl_handle_t h, const void* q_dev, int32_t q_stride, const int32_t* gid_dev, int32_t n_rows,
                      int32_t n, int32_t z_lo, int32_t z_hi, void* stream, int sync);

/* The same build in two calls, so that the halo exchange overlaps its first part: _begin enqueues what needs only
 * the OWNED particles q[0, n_rows) -- the binning of the owned layers, about a tenth of the build -- and may be called
 * while the ghost rows q[n_rows, n) are still being received; _finish (same stream, after the caller has made that
 * stream wait for the exchange) enqueues the rest: the binning of the ghosts, the search, the scan, the expansion.
 * n_ghost_lo = how many of the ghosts lie in the lower neighbour layer (z_lo - 1): the owned particles are placed
 * behind them in the cell-sorted array before any ghost has been seen, so the number is part of the call; it is
 * verified when the ghosts are binned (NL_ERR_DOMAIN).  The result is the one of nl_make_list_slab.  Builds that
 * have nothing to overlap (single rank; NL_BINNING=1) do all their work in _finish. */
int nl_make_list_slab_begin(nl_handle_t h, const void* q_dev, int32_t q_stride, const int32_t* gid_dev, int32_t n_rows,
                            int32_t n, int32_t n_ghost_lo, int32_t z_lo, int32_t z_hi, void* stream);
int nl_make_list_slab_finish(nl_handle_t h, void* stream, int sync);

/* Local-index slab lists, for the consumers below.  Off by default: nothing above changes.
 * While on:
 *   - nl_make_list_slab and nl_make_list_slab_begin take gid_dev == NULL only (a gid array or NL_GID_IN_W: NL_ERR_ARG).
 *     The list is exactly what such a build has always produced: its ids are rows of q_dev, the n_rows owned particles
 *     first and the ghosts behind them, the local-index list of LAMMPS and HOOMD.  Half: row r holds the rows j > r within
 *     the cut-off, so a pair of an owned particle and a ghost is in the owned row on BOTH ranks that see it.  Full: every
 *     owned row holds all its partners, ghosts included.
 *   - nl_lj_forces, nl_lj_virial, nl_pair_histogram and their _enqueue variants accept the list of a slab build that was
 *     made while the switch was on.  The rows are the n_rows owned particles, q_dev holds all n positions of the build, and
 *     partner j is a ghost iff j >= n_rows.  Each family states below what a rank computes; summed over the ranks of a
 *     decomposition the results are those of a whole build of the global box.
 *   - nl_make_list_distributed is NL_ERR_STATE: its lists hold global ids and its ghost counts live on the device.
 *   - Whole builds (nl_make_list, nl_update_list) and their consumers are unaffected.
 * Everything else stays refused by the consumers (NL_ERR_STATE): a slab build made with the switch off, caller ids,
 * distributed builds; a type table, an input-row exclusion table and nl_set_pair_images refuse slab builds as before, so
 * the _typed variants are not reachable on a slab.  A global exclusion table (nl_set_exclusions_global) applies, its ids
 * being the rows of q_dev.
 * Synchronous, as the other setters: finishes a pending build; a changed value drops the list (the next nl_update_list
 * builds); the same value again changes nothing; allocates nothing. */
int nl_set_local_ids(nl_handle_t h, int on);
int nl_get_local_ids(nl_handle_t h, int* on);

/* ------------------------------------------------------------------------------- the decomposed build, whole */

/* The domain-decomposed build with its halo exchange inside the library (no reference
 * counterpart: the reference is single GPU, make_list.cu:122-127).  One process per GPU; rank r of `world` owns the
 * cell layers nl_comm_layers returns for it (contiguous runs of the global mesh's z layers, as even as possible) and
 * passes its owned particles only; per build the library packs the two boundary layers, tells the two z-neighbours how
 * many particles come (the counts change from build to build in a moving system), moves the layers into the ghost rows
 * of the caller's buffer and runs nl_make_list_slab on owned + ghosts.  Point-to-point only, no collective.
 *
 * nl_comm_create: RCCL over xGMI.  unique_id = the NL_UNIQUE_ID_BYTES bytes rank 0 got from nl_comm_unique_id and handed
 *   to every rank out of band (ncclGetUniqueId / ncclCommInitRank).  RCCL is resolved at run time (dlopen: the copy the
 *   process already uses, e.g. PyTorch's, else /opt/rocm/lib): NL_ERR_COMM if it cannot be loaded.  The transfer runs on
 *   a communication stream under the binning of the owned layers (nl_make_list_slab_begin / _finish).
 * nl_comm_create_callbacks: the caller supplies the transport, a blocking host-memory exchange
 *   fn(user, peer_to, send, send_bytes, peer_from, recv, recv_bytes) -> 0 on success, called twice per message round in
 *   the same order on every rank (first everybody sends to rank-1 and receives from rank+1, then the other way; a zero
 *   byte count means that side is skipped).  For MPI / gloo / test harnesses; the layers are staged through pinned host memory.
 * nl_make_list_distributed: q_dev = this rank's positions {x, y, z, w} (stride 4) with the GLOBAL particle id in w
 *   (bit pattern of an int32 for NL_F32, of an int64 for NL_F64: NL_GID_IN_W), n_owned rows filled by the caller and room
 *   for q_capacity rows: the ghosts are written behind the owned rows.  Every owned particle must lie in the rank's
 *   layers (NL_ERR_DOMAIN otherwise: migrating particles between ranks is the caller's job); NL_ERR_CAPACITY when
 *   owned + ghosts exceed q_capacity or the handle's n_max.  Rows (nl_get_half_csr ...) are those of the owned
 *   particles and hold global ids, as after nl_make_list_slab.  With sync == 0 a steady-state build returns without
 *   waiting for the device: the boundary layers travel in messages of negotiated capacity with their counts in a header,
 *   the ghost counts stay on the device (nl_dist.inc).  The first build of a communicator, and the build after one whose
 *   layer outgrew its message (that one reports NL_ERR_CAPACITY at its synchronisation; with sync == 1 it renegotiates and
 *   repeats itself), exchange the counts through the host.
 * nl_distributed_ghosts: the ghost counts of the last build (rows [n_owned, n_owned + lo) and the hi rows behind); waits for
 *   that build.
 * Tested per rank, row by row against the global list, on every search path, mask and capacity edge: tests/test_distributed_paths.py. */
typedef struct nl_comm_s* nl_comm_t;
#define NL_UNIQUE_ID_BYTES 128
typedef int (*nl_sendrecv_fn)(void* user, int peer_to, const void* send, size_t send_bytes, int peer_from, void* recv,
                              size_t recv_bytes);
int nl_comm_unique_id(void* id_out /* NL_UNIQUE_ID_BYTES */);
int nl_comm_create(nl_comm_t* out, int rank, int world, const void* unique_id, int device_id);
int nl_comm_create_callbacks(nl_comm_t* out, int rank, int world, nl_sendrecv_fn fn, void* user, int device_id);
int nl_comm_destroy(nl_comm_t comm);
int nl_comm_layers(nl_handle_t h, nl_comm_t comm, int32_t* z_lo, int32_t* z_hi);
int nl_make_list_distributed(nl_handle_t h, nl_comm_t comm, void* q_dev, int32_t q_capacity, int32_t n_owned, void* stream,
                             int sync);
int nl_distributed_ghosts(nl_comm_t comm, int32_t* n_ghost_lo, int32_t* n_ghost_hi);

/* Waits for the last enqueued build and returns its status (replaces the harness's
 * checkCudaErrors(cudaDeviceSynchronize()), make_list.cu:128). */
int nl_synchronize(nl_handle_t h);

/* ------------------------------------------------------------------------------------ Verlet-skin updates */

/* The Verlet part of the Verlet list (no reference counterpart: its harnesses only build).  The
 * handle's cut-off is rc = the physical cut-off + skin; a list stays valid until some particle has moved more than
 * skin / 2 since its build.  nl_update_list decides that on the device and rebuilds only then, in stream order and with
 * no host involvement, so that an MD step (integrate, nl_update_list, nl_lj_forces_enqueue) can be enqueued ahead and
 * captured into a graph.
 *   nl_set_skin: skin >= 0 (default 0: every particle that moved at all triggers a build); forces the next update to build.
 *   nl_update_list: builds as nl_make_list does (the same list) exactly when
 *     (a) the host knows a reason: no list of an update to keep (first update; nl_initialize, nl_set_list_kind,
 *         nl_set_periodic(_axes), nl_set_offset_width, nl_set_capacity, nl_set_skin, nl_set_pair_images (a changed value),
 *         nl_set_box, nl_set_exclusions(_global), nl_set_type_cutoffs or nl_resort called, or a build other than an update's
 *         run -- nl_make_list, a slab build, nl_profile_stages, nl_profile_last_build -- since; the host has seen the last
 *         build fail) or q_dev, q_stride or n differ from that build's;
 *     (b) the status word of the last performed build is not OK (an asynchronous build that overflowed its capacity);
 *     (c) for some particle i < n, with d = q_now - snap per component in the position type (round to nearest, no
 *         contraction), dd = (double)d, folded to the minimum image on every axis of the nl_set_periodic_axes mask
 *         (dd -= L rint(dd / L), that component only),
 *         r2 = (ddx^2 + ddy^2) + ddz^2 in double without FMA is NaN or > (skin / 2)^2.  snap = the caller's positions
 *         at the last build an update performed, in input order.
 *   Otherwise nothing changes, on the device or the host: the getters, nl_lj_forces and nl_resort see the last build.
 *   sync != 0 behaves like nl_make_list(sync = 1) (grows the list on capacity overflow, returns the status); sync == 0
 *   only enqueues.  An update's build never needs a host re-run (two-pass binning, every launch of its path).  With
 *   nl_set_graph(1) the whole chain (check, gated build, snapshot, result copy) is replayed from one graph.  On a stream
 *   the caller is capturing, an update enqueues plain launches; one that the host would have to force (first build,
 *   growth) or that would wait for another stream is NL_ERR_STATE there.  Slab and distributed builds have no update.
 *   nl_get_update_stats: stats[0] = updates enqueued, stats[1] = builds they performed (device counters, including the
 *   replays of captured updates); waits for the device.
 * Tested on every search path, binning, offset width and list kind, skipped updates byte for byte: tests/test_update_paths.py.
 * Tested in stream order on a caller's non-blocking stream: five steps, each a copy of the positions and an update, enqueued
 * behind one delay while the stream is held, as plain launches and from the handle's graph (captured on the handle's
 * private stream, launched on the caller's): tests/test_caller_stream.py. */
int nl_set_skin(nl_handle_t h, double skin);
int nl_update_list(nl_handle_t h, const void* q_dev, int32_t q_stride, int32_t n, void* stream, int sync);
int nl_get_update_stats(nl_handle_t h, int64_t stats[2]);

/* ------------------------------------------------------------------------------------------------ exclusions */

/* Excluded pairs (no reference counterpart): the bonded partners of a molecular model -- 1-2 and 1-3 pairs of a
 * bead-spring polymer, of water, of any force field with a topology -- left out of the non-bonded list when it is built,
 * as LAMMPS special lists, HOOMD and GROMACS do.  The list is filtered once per build, and every consumer sees it filtered.
 *   The rule: a build with a table leaves out exactly the pairs {i, j} of the table, in either order, and changes nothing
 *     else.  Half list: row min(i, j) loses j; full list: both rows lose the partner.  An excluded pair beyond the cut-off
 *     has no effect.  number_of_partners, key_pointer, npairs / nentries, nl_number_of_pairs, nl_list_checksum,
 *     nl_get_full_transposed and nl_lj_forces(_enqueue) all describe the filtered list.  Holds for F32 and F64, every
 *     periodic mask, 32- and 64-bit offsets and every search path.
 *   nl_set_exclusions: pairs_dev = device int32 [n_pairs][2] of input-order particle indices; n = the particle count of
 *     the builds the table applies to.  The pairs are copied (the caller may free them) and checked on the device:
 *     0 <= i, j < n, i != j, and n <= n_max, else NL_ERR_ARG and the old table is kept.  Duplicates and both orders
 *     are allowed.  The symmetric, sorted, deduplicated table is built on the device; set-up time grows with the square
 *     of the longest row (a wave ranks a row of m ids in m^2 / 64 steps: bonded topologies of a few to a few hundred
 *     partners per particle cost milliseconds, a row of 10^5 ids seconds).  A table that fits the buffers of the one it
 *     replaces is written into them.  Synchronous: waits for the device, finishes a pending build, and forces the next
 *     nl_update_list to build (its reason (a)).  NL_ERR_NOMEM (no room for the pre-exclusion buffers) leaves no table.
 *     n_pairs == 0 or pairs_dev == NULL clears the table: builds are the plain ones again.
 *   nl_get_exclusions: the handle's table as a device CSR, symmetric, per-row ascending, without duplicates:
 *     offsets[n + 1], ids[offsets[n]]; *n_unique = distinct unordered pairs.  NL_ERR_STATE when no table is set.
 *     The pointers stay valid until the table is set, cleared or relabelled.
 *   Builds: a build whose n differs from the table's is NL_ERR_ARG.  Slab builds (nl_make_list_slab with a slab, ids
 *     or the _begin / _finish pair) and distributed builds are NL_ERR_STATE while a table is set.
 *   Capacity is counted BEFORE exclusion: the build writes the unfiltered list first (into a buffer of its own, then a
 *     stage compacts it into the list the getters return), so NL_ERR_CAPACITY and the growth of a synchronous build
 *     follow the unfiltered total.  While a table is set the handle holds a second list of the same capacity and a
 *     second offset array.
 *   Re-sorting: the first nl_resort after a build relabels the table by that build's cell order, once:
 *     (a, b) -> (inv[a], inv[b]) with inv[order[s]] = s, so that the next build excludes the same physical pairs.  This
 *     holds for whatever table is set at that call, also one set after the build (in the order the build was given).
 *     The relabelled table stays in the same device buffers, so a graph the caller captured keeps reading it.  A
 *     caller who permutes its arrays with nl_get_cell_order itself must set the table again.
 *   Builds refuse with NL_ERR_NOMEM while the pre-exclusion buffers could not be (re)allocated.
 *   Graph replays (nl_set_graph, nl_update_list): setting, clearing or relabelling the table captures again.
 *   nl_set_exclusions_global: the table over the ids the list STORES, [0, n_ids), for decomposed runs: the topology in
 *     global tags, the same on every rank, valid while particles migrate (what LAMMPS special lists and HOOMD exclusions
 *     carry).  pairs_dev = device int32 [n_pairs][2] of ids; copied, checked (0 <= a, b < n_ids, a != b, else NL_ERR_ARG
 *     and the old table is kept; duplicates and both orders allowed) and built on the device exactly as above, and as
 *     synchronous.  n_ids is independent of n_max (at most 2147483000): every rank holds the offsets of ALL global ids,
 *     4 bytes per id, plus 4 bytes per table entry (8 per distinct pair); the set-up needs another 12 bytes per id and 8
 *     per entry while it runs.  n_pairs == 0 or NULL clears the table; NL_ERR_NOMEM leaves none; NL_ERR_STATE before
 *     nl_initialize.
 *     One table per handle: nl_set_exclusions and nl_set_exclusions_global replace each other's table, and the handle
 *     remembers which kind it holds.  nl_get_exclusions returns either, with *n = n_ids for a global one.
 *     The rule, in ids: a build with a global table leaves out exactly the entries (row id a, partner id b) with {a, b}
 *     in the table, and changes nothing else.  Half slab build: the row of the smaller id loses the partner, on the rank
 *     that owns that row; full slab build: every owned row loses the partner, ghost partners included.  So the union over
 *     the ranks is the global filtered list entry for entry, and the ranks' nl_list_checksum values sum to its checksum.
 *     number_of_partners, key_pointer, npairs / nentries, nl_number_of_pairs and nl_list_checksum describe the filtered
 *     list; F32 and F64, every periodic mask, both offset widths, every search path.
 *     Builds it applies to: nl_make_list_slab with any id form (NULL = identity, a gid array, NL_GID_IN_W), the _begin /
 *     _finish pair, nl_make_list_distributed (no host synchronisation added), and whole builds, whose ids are their rows.
 *     Where the ids are the rows (gid_dev == NULL) a build needs n_rows <= n_ids, else NL_ERR_ARG at the call.  With
 *     caller ids the stage checks them: a ROW whose id lies outside [0, n_ids) invalidates the build, NL_ERR_ARG reported
 *     where NL_ERR_DOMAIN is (the synchronous return, or the next synchronising call of an asynchronous build).  A
 *     PARTNER id outside the range matches nothing and is kept.  The stage reads the row's id from gid_dev or from the
 *     positions' w: both must stay valid until the build has finished (as they must for nl_list_checksum).
 *     Together with a type table (whole builds only) the pairs go through the typed stage as an input-row table does.
 *     nl_resort NEVER relabels a global table: its ids are the caller's names, not rows.  Capacity is counted before
 *     exclusion as above (NL_ERR_CAPACITY, growth, and the message capacities of a distributed build are untouched).
 *     A table set by nl_set_exclusions (input rows) keeps refusing slab, id and distributed builds with NL_ERR_STATE. */
int nl_set_exclusions(nl_handle_t h, const int32_t* pairs_dev, int64_t n_pairs, int32_t n);
int nl_set_exclusions_global(nl_handle_t h, const int32_t* pairs_dev, int64_t n_pairs, int32_t n_ids);
int nl_get_exclusions(nl_handle_t h, const int32_t** offsets_dev, const int32_t** ids_dev, int32_t* n, int64_t* n_unique);

/* ---------------------------------------------------------------------------------------------- type cut-offs */

/* Per-type cut-offs (no reference counterpart): mixtures whose model sets a cut-off per pair of types (the Kob-Andersen
 * binary glass, coarse-grained beads of several sizes, solvent around solutes), as LAMMPS pair_coeff and HOOMD r_cut do.
 * The search still runs at the handle's rc; a stage behind it (the one of the exclusions) keeps what the table allows.
 *   The rule: with a table set, a build keeps an entry (row i, partner j) of the list it would build without the table
 *     iff !(r2 > rc2[t_i][t_j]).  r2 is the value the search tested for that entry: (dx*dx + dy*dy) + dz*dz in the
 *     position type T without FMA, at the image the search used (a wrapped particle's stored image, the -+L shift of a
 *     periodic face rounded to T first); rc2[a][b] is the largest T <= rc_ab * rc_ab in double (the rounding of rc).
 *     So all rc_ab == rc is the plain list, and rc_ab == 0 keeps only coincident pairs of that type pair.  Half list:
 *     the row min(i, j) decides; full list: each row decides with its own r2 (across a periodic face the two rows may
 *     disagree within one ulp, as the full list itself may).  With an exclusion table as well, one stage applies both:
 *     an entry is kept if it is not excluded and within its rc_ab.  number_of_partners, key_pointer, npairs / nentries,
 *     nl_number_of_pairs, nl_list_checksum, nl_get_full_transposed and nl_lj_forces(_enqueue) describe the filtered list.
 *   nl_set_type_cutoffs: types_dev = device int32 [n] in input order (copied: the caller may free it), checked on the
 *     device, 0 <= t < ntypes, and n <= n_max; ntypes = 1 .. NL_MAX_TYPES; rc_host = ntypes x ntypes doubles,
 *     row-major, exactly symmetric, each in [0, rc] (the skin included, as in rc).  Anything else, NaN included, is
 *     NL_ERR_ARG and the old table is kept.  types_dev == NULL or ntypes == 0 clears the table.  Synchronous: waits for
 *     the device, finishes a pending build, and forces the next nl_update_list to build (its reason (a)).
 *   nl_get_types: the handle's copy of the types (relabelled by a re-sort), n and ntypes; NL_ERR_STATE without a table.
 *   As with the exclusion table: a build whose n differs from the table's is NL_ERR_ARG; slab and distributed builds are
 *     NL_ERR_STATE while a table is set; capacity is counted before filtering (NL_ERR_CAPACITY and growth follow the
 *     unfiltered total); the first nl_resort after a build permutes the types by that build's cell order,
 *     types[s] <- types[order[s]], in the same buffer; setting, clearing or relabelling captures graphs again.
 *     Builds without a table launch nothing of this. */
#define NL_MAX_TYPES 32
int nl_set_type_cutoffs(nl_handle_t h, const int32_t* types_dev, int32_t n, int32_t ntypes, const double* rc_host);
int nl_get_types(nl_handle_t h, const int32_t** types_dev, int32_t* n, int32_t* ntypes);

/* ---------------------------------------------------------------------------------------------- pair images */

/* The periodic image of every entry of the list (no reference counterpart: its box is open), as ASE / matscipy
 * neighbour_list("ijS"), the edge_index + shifts tensors of machine-learned potentials and LAMMPS image flags report it.
 *   The rule: for an entry (row i, partner j) of the list the getters return, the image is the integer triple
 *       s = n_j + w_ij - n_i
 *     n_p = the wraps of particle p, as the binning decides them from the input coordinate (nl_set_box: n_p[d] in
 *       {-1, 0, +1} on an axis of the nl_set_periodic_axes mask, 0 on an open axis);
 *     w_ij[d] = -1 where i's cell is the first along d and j's the last, +1 the other way round, else 0 (axes of the mask
 *       only): the face through which the search staged j.
 *     So |s[d]| <= 3, and s[d] = 0 on an open axis and in the open box (mask 0).
 *     Meaning: q_j + S(s) - q_i, S(s) = s_a a + s_b b + s_c c over the build's box, is the displacement at which the search
 *     found the pair; with m_d >= 3 it is the only image within rc.  The two rows of a full list give s_ji = -s_ij exactly
 *     (both terms are antisymmetric).
 *   Storage: 4 bytes per entry, int8 {s_a, s_b, s_c, 0}, at the index of the entry in sorted_list / list (both offset widths).
 *   nl_set_pair_images: off by default.  Synchronous, as the other setters: finishes a pending build; a changed value drops
 *     the list, makes the next nl_update_list build and captures graphs again; the same value again changes nothing.  While on, the handle holds one more buffer of
 *     capacity x 4 bytes (and 2 bytes per particle), allocated, estimated and grown wherever the list is; NL_ERR_NOMEM
 *     leaves the flag off.  Slab builds (a slab, ids, the _begin / _finish pair) and distributed builds are NL_ERR_STATE
 *     while it is on.  Builds with the flag on run one more stage at their very end, behind the filter stage of an
 *     exclusion or type table: the images describe the filtered list.  Builds with the flag off launch nothing of this.
 *   nl_get_pair_images: the images of the last build, *nentries of them (npairs / nentries of nl_get_*_csr); synchronises;
 *     NL_ERR_STATE when the flag is off or there is no build.  The pointer is valid until the next build.
 *   nl_update_list while the flag is on: rule (c) is taken WITHOUT the fold to the minimum image (the open-box form, on
 *     every axis).  A particle that the caller wrapped back into the box has moved by a box vector, which is longer than
 *     skin / 2: the update builds, and the images are computed again.  Images are therefore valid for the positions of the
 *     build and for any continuation of them within the skin; a list with the flag on never outlives a re-wrap.  A skipped
 *     update leaves the list and the images as they are.  With the flag off rule (c) is unchanged.
 *   nl_pair_vectors: the consumer.  out_dev[k] = {dx, dy, dz, r2} in the position type T for every entry k of the last
 *     build, from q_dev (the build's positions, or positions moved within the skin; same dtype, q_stride 3 or 4):
 *     S(s) in double as ((s_a Lx + s_b xy) + s_c xz, s_b Ly + s_c yz, s_c Lz), each component rounded to T once;
 *     d_c = (S_c == 0 ? q_j[c] : q_j[c] + (T)S_c) - q_i[c], one rounding per operation; r2 = (dx*dx + dy*dy) + dz*dz without
 *     FMA.  The sign is r_j - r_i (the ASE convention).  This r2 is NOT the r2 the search tested: the search rounds the wrap
 *     and the face shift separately, so the two may differ in the last place, and no claim r2 <= rc2 is made.  Needs the
 *     flag on, a single-device build and ids that index q (else NL_ERR_STATE); waits for the build first.
 *   nl_pair_vectors_enqueue: without the wait, stream-ordered behind the last nl_update_list on the same stream (or behind a
 *     build that has been synchronised), with the rules of nl_lj_forces_enqueue: a pending plain asynchronous build is
 *     NL_ERR_STATE; where the build's status word says the list is invalid the vectors are NaN and the error surfaces at
 *     the next nl_synchronize.  out_dev must hold the list's capacity (nl_set_capacity), since the host does not know the
 *     number of entries yet.  Copies nothing from the host: it can be captured. */
int nl_set_pair_images(nl_handle_t h, int on);
int nl_get_pair_images(nl_handle_t h, const int8_t** images_dev, int64_t* nentries);
int nl_pair_vectors(nl_handle_t h, const void* q_dev, int32_t q_stride, void* out_dev, void* stream);
int nl_pair_vectors_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------- results */

/* The CPU class's accessors (neighlist_cpu.hpp:437-463): key_pointer()[N+1], sorted_list()[P],
 * number_of_partners()[N] (half counts, on min(i,j)), number_of_pairs() = P -- as DEVICE pointers.
 * Partners of particle i are sorted_list[key_pointer[i] .. key_pointer[i+1]), in no particular order (the
 * reference's order is its visit order; its own check sorts each segment first, make_list.cpp:120-128,211).
 * Synchronises. Any out pointer may be NULL. */
int nl_get_half_csr(nl_handle_t h, const int32_t** key_pointer_dev, const int32_t** sorted_list_dev,
                    const int32_t** number_of_partners_dev, int64_t* npairs);

/* The same arrays of a NL_LIST_FULL build: key_pointer[N+1], list[2P], full counts [N]; *nentries = 2P.
 * NL_ERR_STATE if the last build was a half build (and nl_get_half_csr after a full build). */
int nl_get_full_csr(nl_handle_t h, const int32_t** key_pointer_dev, const int32_t** list_dev,
                    const int32_t** number_of_partners_dev, int64_t* nentries);

/* The same lists with 64-bit offsets: key_pointer[N+1] as int64 (no reference counterpart: its offsets are int32,
 * neighlist_cpu.hpp:29, and BASELINE config 4's 2.5e9 pairs do not fit them). */
int nl_get_half_csr64(nl_handle_t h, const int64_t** key_pointer_dev, const int32_t** sorted_list_dev,
                      const int32_t** number_of_partners_dev, int64_t* npairs);
int nl_get_full_csr64(nl_handle_t h, const int64_t** key_pointer_dev, const int32_t** list_dev,
                      const int32_t** number_of_partners_dev, int64_t* nentries);

/* Order-independent checksum of the list of the last build, computed on the device: the wrapping sum over entries
 * (row i, partner j) of mix((id_i << 32) | j), mix(v): v *= 0x9E3779B97F4A7C15; v ^= v >> 29 -- the pair-set hash of
 * the reference harness's known answers -- with id_i the row's global id (slab builds: the ids the
 * build was given).  The sum over the ranks of a decomposed build is the checksum of the global list.  Synchronises. */
int nl_list_checksum(nl_handle_t h, uint64_t* checksum, int64_t* nentries);

/* The GPU class's accessors neigh_list() / number_of_partners() (neighlist_gpu.hpp:468-482): the FULL list in
 * the transposed layout list[k * row_stride + i], k < count[i], original particle ids: converted from the full
 * CSR of a NL_LIST_FULL build (one coalesced pass), or derived on the device from the half list of a NL_LIST_HALF
 * build (scattered writes: about ten times slower).  Entries k >= count[i] hold -1 when the buffer is first
 * allocated or grown and whatever an earlier build left there afterwards (the reference fills -1 once in
 * Initialize and never again, neighlist_gpu.hpp:271); after a NL_LIST_HALF build the buffer is filled anew by every
 * fetch that follows a build.  nl_initialize and nl_set_list_kind drop the buffer: the next fetch allocates and fills
 * it.  *row_stride is the n of the last build and changes with it (the buffer is kept while it holds rows x n
 * entries); *max_partners receives max_i count[i].  A second call after the same build returns the same pointers
 * without running a kernel.  Synchronises.
 * Whole single-device builds only: after a slab or distributed build, whose ids are global and not row indices,
 * NL_ERR_STATE.
 * Tested (tests/test_handle_resize.py) on one handle across nl_initialize growth and builds of 0 to 12 000 particles,
 * from half and full builds: counts, sorted columns, shape, padding where promised and the pair-set hash against the
 * oracle; blocks of one build on both sides of the flat kernel's LDS piece; kind switches; wide offsets. */
int nl_get_full_transposed(nl_handle_t h, const int32_t** list_dev, const int32_t** count_dev, int64_t* row_stride,
                           int32_t* max_partners);

/* number_of_pairs(): P, the half-pair count (neighlist_cpu.hpp:437-439).  The GPU class returns the sum of the
 * full counts = 2P (neighlist_gpu.hpp:484-487); the C++ shim doubles it.  Synchronises. */
int nl_number_of_pairs(nl_handle_t h, int64_t* npairs);

/* ------------------------------------------------------------------------------------- periodic re-sorting */

/* The physical re-sort the reference declares and never performs: SORT_FREQ = 50 (neighlist_gpu.hpp:72), CopyGather
 * (neighlist_gpu.hpp:144-151), SortPtclData (neighlist_cpu.hpp:176-180, its call commented out at :421).  A build
 * already sorts a COPY of the positions into cell order; an MD loop that permutes its own per-particle arrays the same
 * way every SORT_FREQ builds keeps them spatially coherent, which makes the binning pass of the next builds and every
 * gather through the list (forces) faster.
 *   nl_get_cell_order: order[s] = input index of the particle the last build placed at cell-ordered slot s
 *     (the reference's ptcl_id_in_mesh, neighlist_gpu.hpp:153-199), a device pointer valid until the next build.
 *   nl_resort: array[s] <- array[order[s]] in place for one per-particle array of elem_bytes (4, 8, 12, 16, 24 or 32)
 *     per particle: positions, velocities, ids, ... -- call it once per array, then rebuild: the new list is the list
 *     of the permuted particles (indices are the NEW positions in the arrays).  Enqueued on `stream`; single-device
 *     builds only.  Synchronises with the last build first (on the host: the permutation is that build's result; the
 *     relabelling of an exclusion or type table runs on a private stream and is waited for), then gathers and copies back
 *     on `stream`, ordered behind whatever wrote the array there.
 *     Tested on a caller's held non-blocking stream, the arrays written behind the delay, followed by a rebuild on that
 *     stream, with and without the tables: behind a synchronised build, where the calls only enqueue (the first re-sort
 *     after a build relabels the tables and waits for the device; later ones do not), and behind an asynchronous build,
 *     which is waited for: tests/test_caller_stream.py. */
int nl_get_cell_order(nl_handle_t h, const int32_t** order_dev, int32_t* n);
int nl_resort(nl_handle_t h, void* array_dev, size_t elem_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------- a consumer */

/* Truncated Lennard-Jones forces from the list of the last build (the reference stops at
 * the list: its momentum array is allocated and never used, make_list.cpp:135,138-140).  q_dev: the positions the
 * list was built from (or moved by less than the skin), same dtype and stride; f_dev: n x 4 values of that dtype,
 * {fx, fy, fz, pe_i} with pe_i = half the pair energies of particle i; pairs beyond rc_force (<= the list's cut-off)
 * are skipped; distances are taken as the list took them: between the coordinates as given (open box, the reference's
 * rule) or at the minimum image on the axes of the build's nl_set_periodic_axes mask, each component on its own.
 * Positions may lie up to one box length outside the box, as for the builds (positions that drift and are never wrapped,
 * nl_update_list with nl_set_pair_images): the separation is taken with its rounding error and folded with rint,
 * d -= L rint(d / L) in z, y, x order with the tilts, so a force does not depend on which image a coordinate sits in.
 * The box is the build's, rounded to the position type like everything the library does with it.
 * Tested contract (tests/test_lj_consumer.py): every component of every particle within c u S of an O(N^2) float64 sum,
 * S the uncancelled sum of that component's pair terms, u the unit roundoff of the position type; rc_force is exact for
 * pairs further than 64 ulp (in r) from it.  After a NL_LIST_FULL build every row gathers its partners and
 * writes its force once; after a NL_LIST_HALF build every pair is evaluated once and the reaction is added to the
 * partner with floating-point atomics (f_dev is zeroed first).  Enqueued on `stream` (NULL = the null stream);
 * waits for the build first -- on the host, whichever stream the build was enqueued on, so the call may be made on another
 * stream than the build's.  Tested for every consumer (Lennard-Jones, pair table, EAM, Stillinger-Weber, Coulomb, the
 * excluded-pair term, the histogram, nl_pair_vectors) from the null stream and from a second non-blocking stream behind an
 * asynchronous build on a held stream: tests/test_caller_stream.py.
 * On a local-index slab list (nl_set_local_ids): f_dev is n_rows x 4, q_dev holds the n positions of the build.  Per entry
 * (row i owned, partner j; j is a ghost iff j >= n_rows): a full list is read as ever; in a half list an owned partner
 * receives the reaction, a ghost partner receives nothing -- its owner evaluates the same pair in its own row, so there are
 * no atomics to ghost rows and no reverse communication; pe_i takes half the pair energy either way.  Every owned
 * particle's {fx, fy, fz, pe_i} is what a whole build of the global box gives that particle; the pe_i of all ranks sum to U. */
int nl_lj_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force,
                 void* f_dev, void* stream);
/* nl_lj_forces without the wait: stream-ordered behind the last nl_update_list, which must have been enqueued on the same
 * stream (or behind a build that has been synchronised); a pending plain asynchronous build is NL_ERR_STATE.
 * rc_force <= rc - skin (what a list reused within the skin guarantees), else NL_ERR_ARG.  Where the build's status word
 * says the list is invalid the forces are NaN; the error itself surfaces at the next nl_synchronize.
 * Only enqueues: on a handle whose calls have all run once (nothing left to allocate) it returns while the stream is still
 * held back.  Tested for every consumer's enqueue variants behind an update on a caller's held non-blocking stream, the
 * positions and charges written behind the delay: tests/test_caller_stream.py. */
int nl_lj_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force,
                         void* f_dev, void* stream);
/* Typed Lennard-Jones for a list built with a type table: epsilon, sigma and rc_force of a pair are [t_i][t_j] of
 * ntypes x ntypes row-major, exactly symmetric matrices (sigma > 0, rc_force > 0, rc_force_ab <= rc_ab, finite
 * epsilon; else NL_ERR_ARG).  A pair of types with rc_ab = 0 has no entries: its rc_force_ab is 0, and it adds nothing.  nl_set_lj_type_params copies them to the device synchronously; its ntypes must be the type
 * table's (NL_ERR_STATE without a table).  nl_lj_forces_typed(_enqueue) compute what nl_lj_forces(_enqueue) compute,
 * with the same lists, masks, NaN rule and ordering, from those parameters; NL_ERR_STATE while the table or the
 * parameters are missing, NL_ERR_ARG when they no longer match (ntypes, rc_force_ab > rc_ab), and the enqueue variant
 * also needs rc_force_ab <= rc_ab - skin.  The enqueue variant copies nothing from the host: it can be captured. */
int nl_set_lj_type_params(nl_handle_t h, int32_t ntypes, const double* epsilon, const double* sigma, const double* rc_force);
int nl_lj_forces_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_lj_forces_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);

/* The totals that belong to those forces: the virial tensor W, the potential energy U and the number of interacting pairs,
 * for a pressure P = N k_B T / V + (W_xx + W_yy + W_zz) / (3 V).  out_dev: 8 doubles on the device, for both position
 * types: {W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}.  The rule:
 *   - The sum runs over the entries (row i, partner j) of the list of the last build: the filtered list where an
 *     exclusion or type table is set.
 *   - For each entry d comes from the image rule and fx, fy, fz, pe, in from the pair function of nl_lj_forces (lj_image,
 *     lj_pair), with the same rc_force and parameter handling.
 *   - The entry's terms are computed in the position type, one rounding each, without contraction: fx dx, fy dy, fz dz,
 *     fx dy, fx dz, fy dz; pe (the pair's full energy); 1 if in (0 < r^2 < rc_force^2), else nothing.
 *   - Each term is converted to double and summed in double.
 *   - After a NL_LIST_HALF build every entry counts once, after a NL_LIST_FULL build 1/2 (exact), so both list kinds
 *     report W_ab = sum over pairs d_a F_b, U = sum over pairs u(r), n_in = the number of pairs within rc_force.
 *   - Sign: d = r_i - r_j and F the force on i, so repulsion gives positive diagonal terms (the LAMMPS convention).
 *   - Ordering, the state required, the rc_force <= rc test (<= rc - skin for the enqueue variants) and the typed
 *     variants' conditions are exactly those of the four force calls; slab and distributed builds: NL_ERR_STATE (but for a
 *     local-index slab list, below).
 *   - Where the enqueue variants find a non-zero status word all 8 values are NaN; the error itself surfaces at the next
 *     nl_synchronize.  n == 0 gives 8 zeros.
 *   - Reproducible: no floating-point atomics anywhere, every sum has a fixed order.  Two calls on the same list and
 *     positions on the same device give the same 8 doubles, bit for bit.  (Half and full builds of the same input order
 *     their sums differently and agree within the bound below, not bit for bit.)
 *   - Rows are dealt to one wave each over a grid of min(ceil(n / 4), NL_VIRIAL_BLOCKS) blocks of 4 waves; each block
 *     leaves one partial of 8 doubles in a scratch buffer of the handle, which a second kernel adds up.  The first call
 *     allocates that buffer: on a stream that is being captured it returns NL_ERR_STATE (call once before the capture).
 *     Calls on one handle share it, so they must be ordered against each other, as everything else on a handle: two calls
 *     of any totals on two streams need the caller's fence (an event recorded behind the first, waited for by the second
 *     stream); the library adds none.  Tested fenced, two enqueue variants on two streams: tests/test_caller_stream.py.
 *   - The enqueue variants copy nothing from the host and can be captured, as nl_lj_forces_enqueue.
 *   - On a local-index slab list (nl_set_local_ids) the rows are the n_rows owned particles and every entry (row i owned,
 *     partner j; j is a ghost iff j >= n_rows) has a weight, applied in double: after a NL_LIST_FULL build 1/2 for every
 *     entry, as above; after a NL_LIST_HALF build 1 for an owned partner and 1/2 for a ghost partner, whose owner stores
 *     the pair too.  The weights are powers of two (exact), n_in may be a half-integer on a rank, and the 8 doubles summed
 *     over the ranks of a decomposition are W, U and n_in of the global box.  Reproducible as above.
 * Tested contract (tests/test_lj_virial.py): every component within c_W u S of an O(N^2) float64 sum,
 * S that component's uncancelled sum; n_in exact where no pair lies within 2^-17 (relative, r^2) of a cut-off. */
#define NL_VIRIAL_BLOCKS 2048
int nl_lj_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force,
                 double* out_dev, void* stream);
int nl_lj_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double epsilon, double sigma, double rc_force,
                         double* out_dev, void* stream);
int nl_lj_virial_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);
int nl_lj_virial_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);

/* Tabulated pair potentials: the forces and totals above for any pair potential the caller has sampled (Morse, Buckingham,
 * Yukawa, a switched WCA, a coarse-grained or force-matched model), as LAMMPS pair_style table, HOOMD pair.Table and the
 * GROMACS user tables do it: the caller samples once, the kernel interpolates.  The rule:
 *   - Knots, uniform in r^2 so that no pair needs a square root.  In double D = (r_max^2 - r_min^2) / (nknots - 1) and
 *     x_k = r_min^2 + k D.  The caller passes F[slot][k] = -U'(r) / r and U[slot][k] = U(r) at r = sqrt(x_k): F is the force
 *     over r, so the force on i is F d with d = r_i - r_j.  Both arrays are nslots x nknots doubles, row-major, finite.  The
 *     energy shift is the caller's business: U(r_max) need not be 0.
 *   - Slots.  ntypes = 1: one table for every pair, with or without a type table set.  ntypes > 1 needs a type table
 *     (nl_set_type_cutoffs) of exactly that ntypes, checked at the calls: nslots = ntypes (ntypes + 1) / 2 and a pair reads
 *     slot(a, b) of nl_pair_histogram_typed.  One grid (r_min, r_max, nknots) serves all slots; a pair of types with a
 *     shorter range pads its table with zeros.
 *   - Device form, in the position type T: each knot holds {F_k, dF_k, U_k, dU_k} with dF_k = (T)(F[k + 1] - F[k]), the
 *     difference taken in double and rounded once, dU_k the same, and 0 for the last knot.  x0 = (T)(r_min^2),
 *     xc = (T)(r_max^2), iD = (T)(1 / D).
 *   - Per entry: d from the image rule of nl_lj_forces; r2 = dx dx + dy dy + dz dz as the Lennard-Jones pair function writes
 *     it, without contraction; in = r2 < xc && r2 > 0; outside `in` everything is 0.  For a pair that is in, all in T with one
 *     rounding per operation: s = (r2 - x0) iD, k = min((int)s, nknots - 2), t = s - (T)k, fr = F_k + t dF_k,
 *     pe = U_k + t dU_k, (fx, fy, fz) = fr d.
 *   - Below the table.  A pair that is in with r2 < x0 has no value: its fr and pe are NaN, and the NaN reaches both
 *     particles' forces (half list: the row's and the partner's; full list: each one's own row) and all 8 totals, n_in
 *     included.  Deliberately so: a clamp would be silently wrong physics, and an error word would need a host sync.
 *   - nl_set_pair_table: 2 <= nknots <= NL_TABLE_MAX_KNOTS, 0 < r_min < r_max, finite values, 1 <= ntypes <= NL_MAX_TYPES,
 *     else NL_ERR_ARG and the old table is kept.  nknots == 0, or F_host and U_host both NULL, clears the table (one of them
 *     alone NULL is NL_ERR_ARG).  Synchronous, as nl_set_lj_type_params: it waits for the device and copies.  The device
 *     buffer is kept where the new table fits, so a captured graph keeps reading it (and reads the new table).  The list
 *     is not touched: nl_update_list is not forced to build.  nl_get_pair_table: NL_ERR_STATE while no table is set.
 *   - Reach, at the calls: r_max <= rc for the synchronous calls and rc - skin for the enqueue calls; with a type table
 *     r_max <= rc_ab (less the skin) for every pair of types with rc_ab > 0 -- a pair with rc_ab = 0 has no entries.  Else
 *     NL_ERR_ARG.  NL_ERR_STATE while no table is set, or while a table of ntypes > 1 has no type table.
 *   - Everything else is nl_lj_forces / nl_lj_virial and their _enqueue variants: ordering and required state, NaN on a
 *     non-zero status word, the layouts of f_dev (n_rows x 4 of T: fx, fy, fz, pe_i) and out_dev (8 doubles), the half
 *     list's reaction with atomics after zeroing f_dev, full-list rows written once, the factor 1/2 of a full list, the
 *     ghost rules of a local-index slab list (there only ntypes = 1 is reachable: type tables refuse slab builds), the
 *     shared scratch of the totals with its first-call allocation rule, and totals that are reproducible bit for bit.
 *     The enqueue variants copy nothing from the host and can be captured.
 *   - Kernels.  One wave per row over a persistent grid of min(ceil(n_rows / 4), NL_TABLE_BLOCKS) blocks of 4 waves, whose
 *     waves take the rows 4 block + wave, + 4 blocks, ...  A table of at most NL_TABLE_LDS_BYTES (nslots x nknots x 4 x
 *     sizeof(T)) is staged into LDS once per block; a larger one is read from global memory.  Both paths compute the same
 *     bits; NL_TABLE_LDS=0 in the environment of nl_set_pair_table forces the global path for that table (tests, A/B).
 * Tested contract (tests/test_pair_table.py): every component of every particle within TABLE_C u S,
 * and the totals within c_W u S, of an O(N^2) float64 sum of the same interpolation rule on the caller's double tables,
 * S the uncancelled sums including the conditioning of s on the rounding of r2. */
#define NL_TABLE_MAX_KNOTS 4096
#define NL_TABLE_BLOCKS 512       /* most blocks of the table kernels */
#define NL_TABLE_LDS_BYTES 65280  /* largest table staged in LDS: 64 KiB less the 256 bytes of the totals' block partials */
int nl_set_pair_table(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min, double r_max, const double* F_host,
                      const double* U_host);
int nl_get_pair_table(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min, double* r_max);
int nl_table_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_table_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_table_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);
int nl_table_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);

/* Embedded-atom potentials (LAMMPS pair_style eam, eam/alloy; HOOMD metal.EAM): forces, per-particle energies and the 8
 * totals of E = sum_i F_{t_i}(rho_i) + sum_pairs phi(r), rho_i = sum_j f_{t_j}(r_ij), j the partners of i in the list.  The rule:
 *   - Pair part.  phi is the handle's pair table (nl_set_pair_table), evaluated by exactly the rule stated there, slots and
 *     all: fr_phi, pe_phi, in_phi.  It must be set (NL_ERR_STATE otherwise); a model without a pair part passes zeros.
 *   - Density tables.  The grid rule of nl_set_pair_table on a grid of their own: D = (r_max_d^2 - r_min_d^2) / (nknots_d - 1),
 *     x_k = r_min_d^2 + k D.  One slot per type b of the SOURCE particle: ntypes slots.  The caller passes f[b][k] = f_b(r) and
 *     G[b][k] = -f_b'(r) / r at r = sqrt(x_k), ntypes x nknots_d doubles each, row-major, finite.  Device form: the knot
 *     {G_k, dG_k, f_k, df_k} in the position type T, differences taken in double and rounded once, 0 at the last knot;
 *     x0_d = (T)(r_min_d^2), xc_d = (T)(r_max_d^2), iD = (T)(1 / D).  With r2 of the entry: in_d = r2 < xc_d && r2 > 0;
 *     s = (r2 - x0_d) iD, k = min((int)s, nknots_d - 2), t = s - (T)k, one rounding per operation; f = f_k + t df_k and
 *     G = G_k + t dG_k.  Outside in_d a partner contributes nothing.  A pair that is in_d with r2 < x0_d has no value: NaN, by
 *     the same deliberate rule as a pair below the pair table.
 *   - Embedding tables.  One slot per type a, uniform in rho on [0, rho_max]: rho_k = k Drho, Drho = rho_max / (nknots_e - 1)
 *     in double.  The caller passes E[a][k] = F_a(rho_k) and P[a][k] = F_a'(rho_k).  Device form {E_k, dE_k, P_k, dP_k} in T,
 *     rounded as above; iDrho = (T)(1 / Drho), rmax = (T)rho_max.  Per particle, in T with one rounding per operation:
 *     s = rho iDrho, k = min((int)s, nknots_e - 2), t = s - (T)k, Fe = E_k + t dE_k, fp = P_k + t dP_k.  rho outside
 *     0 <= rho <= rmax, or NaN, gives Fe = fp = NaN: a clamp would be silently wrong physics.
 *   - Densities.  rho_i is the sum in T of f_{t_j}(r2) over the entries of i.  After NL_LIST_FULL row i gathers its partners
 *     and is written once.  After NL_LIST_HALF rho is zeroed, every entry (row i, partner j) adds f_{t_j} to the row's sum and
 *     f_{t_i} to rho_j with a floating-point atomic, and the row's sum reaches rho_i with one atomic.
 *   - Forces.  For an entry (row i, partner j): d from the image rule of nl_lj_forces, r2 = dx dx + dy dy + dz dz without
 *     contraction; G_i = the density slot t_i at r2, G_j = the slot t_j; emb = fp_i G_j + fp_j G_i where in_d, else 0 (taken
 *     only where in_d, not as a product with 0: a NaN fp reaches the partners within r_max_d and nobody else);
 *     fr = fr_phi + emb, one rounding per operation, no FMA; (fx, fy, fz) = fr d, the force on i, d = r_i - r_j;
 *     in = in_phi || in_d.  f_dev is n x 4 of T: {fx, fy, fz, pe_i}, pe_i = (half the pair energies pe_phi, as
 *     nl_table_forces) + Fe_i, Fe_i added last with one rounding, so sum pe_i = E.  The half list's reaction is
 *     nl_table_forces': atomics after zeroing.
 *   - Totals, the 8 doubles of nl_lj_virial: W_ab = sum_pairs d_a (fr d_b), U = sum_pairs pe_phi + sum_i Fe_i, n_in = the
 *     pairs with `in`.  Terms in T, converted and summed in double in a fixed order as nl_lj_virial's; each Fe_i enters a
 *     double sum of its own once, whatever the list kind (it is not halved after a full build).
 *   - NaN.  A NaN fp_i (rho_i out of range) reaches i's own force and energy, the force of every partner within r_max_d and all
 *     8 totals; a pair below r_min_d reaches both densities and from there the same places.
 *   - Reproducibility.  After NL_LIST_FULL no pass uses an atomic: two calls on the same list and positions give the same
 *     bits -- forces, rho and the 8 totals.  After NL_LIST_HALF rho is summed by atomics, so rho and EVERYTHING that follows,
 *     the 8 totals included, is reproducible only within the tested bound: nl_eam_virial does not inherit nl_lj_virial's
 *     bit-for-bit promise on a half list.
 *   - Types.  ntypes == 1: one density and one embedding slot, with or without a type table.  ntypes > 1 needs a type table
 *     of exactly that ntypes (NL_ERR_STATE without one, NL_ERR_ARG for another ntypes) and a pair table of 1 or ntypes types.
 *   - Reach, at the calls: r_max of the pair table and r_max_d <= rc for the synchronous calls, <= rc - skin for the enqueue
 *     calls; with a type table <= rc_ab (less the skin) for every rc_ab > 0.  Else NL_ERR_ARG.
 *   - nl_set_eam: 2 <= nknots_d, nknots_e <= NL_TABLE_MAX_KNOTS, 0 < r_min_d < r_max_d, rho_max > 0, 1 <= ntypes <=
 *     NL_MAX_TYPES, finite values everywhere, else NL_ERR_ARG and the old tables are kept.  nknots_d == 0, nknots_e == 0 or
 *     four NULL arrays clear the tables (some of them NULL: NL_ERR_ARG).  Synchronous; the device buffer is kept where the new
 *     tables fit, as nl_set_pair_table's; the list is not touched.  nl_get_eam: the scalars, and whether the density pass
 *     (lds_density) and the forces and totals (lds_forces) read their tables from LDS; NL_ERR_STATE while no tables are set.
 *   - Scratch.  rho, fp and Fe (3 T per particle, sized by n_max) belong to the handle.  The first of the four calls allocates
 *     them: on a stream that is being captured it returns NL_ERR_STATE (call once before the capture), the rule of the
 *     totals' scratch, which nl_eam_virial shares.  nl_initialize drops them.  nl_eam_get_density: rho_i and fp_i = F'(rho_i)
 *     of the last call in T, in row order, valid until the next call or nl_initialize, stream-ordered behind that call
 *     (no wait); NL_ERR_STATE before the first call.
 *   - Slab and distributed builds: NL_ERR_STATE, local-index slab lists (nl_set_local_ids) included.  The force on an owned
 *     particle needs fp of its ghost partners, a forward halo exchange of fp between the two passes that is the caller's.
 *   - Kernels.  The persistent grid of the table kernels.  Density pass: its table in LDS where it fits NL_TABLE_LDS_BYTES;
 *     embedding: one thread per particle, table from global memory; forces and totals: the pair table and the density table
 *     both in LDS where together they fit NL_TABLE_LDS_BYTES, else both from global memory.  NL_TABLE_LDS=0 in the environment
 *     of nl_set_eam forces the global path of all three.  Both paths compute the same bits.
 *   - Everything else (ordering, state, NaN on a non-zero status word, n == 0, the enqueue variants copy nothing and can be
 *     captured) is nl_table_forces' / nl_table_virial's.
 * Tested contract (tests/test_eam.py): rho within EAM_C_RHO u S_rho, every component of every particle
 * within EAM_C u S and the totals within EAM_CW u S of an O(N^2) float64 evaluation of the same rule, S the uncancelled sums
 * including the conditioning of fp and Fe on rho. */
int nl_set_eam(nl_handle_t h, int32_t ntypes, int32_t nknots_d, double r_min_d, double r_max_d, const double* f_host,
               const double* G_host, int32_t nknots_e, double rho_max, const double* E_host, const double* P_host);
int nl_get_eam(nl_handle_t h, int32_t* ntypes, int32_t* nknots_d, double* r_min_d, double* r_max_d, int32_t* nknots_e,
               double* rho_max, int32_t* lds_density, int32_t* lds_forces);
int nl_eam_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_eam_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_eam_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);
int nl_eam_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);
int nl_eam_get_density(nl_handle_t h, const void** rho_dev, const void** fp_dev, int32_t* n);

/* Stillinger-Weber three-body potentials (LAMMPS pair_style sw, HOOMD md.many_body.SW: silicon, germanium, mW water, CdTe, GaN,
 * SiC): forces, per-particle energies and the 8 totals of
 *   E = sum_pairs phi(r) + sum_i sum_{j<k} Lambda[t_i][t_j][t_k] (cos theta_jik - c0[t_i][t_j][t_k])^2 g_{t_i t_j}(r_ij) g_{t_i t_k}(r_ik),
 * j, k the partners of the centre i in the list.  The rule, for both position types T, with one rounding per operation, no
 * contraction, and sqrt and / the correctly rounded IEEE operations (the compiler's default for HIP in fp32 as in fp64):
 *   - Pair part.  phi is the handle's pair table (nl_set_pair_table), evaluated by exactly the rule stated there, slots and
 *     all: fr_phi, pe_phi, in_phi.  It must be set (NL_ERR_STATE otherwise); a model without a pair part passes zeros.
 *   - Radial tables g.  The grid rule of nl_set_pair_table on a grid of their own: D = (r_max_3^2 - r_min_3^2) / (nknots - 1),
 *     x_k = r_min_3^2 + k D.  ntypes x ntypes slots, slot a ntypes + b for centre type a and end type b (it need not be
 *     symmetric).  The caller passes g[slot][k] = g(r) and G[slot][k] = -g'(r) / r at r = sqrt(x_k), finite.  Device form: the
 *     knot {G_k, dG_k, g_k, dg_k} in T, differences taken in double and rounded once, 0 at the last knot; x0_3 = (T)(r_min_3^2),
 *     xc_3 = (T)(r_max_3^2), iD = (T)(1 / D).  in_3 = r2 < xc_3 && r2 > 0; s = (r2 - x0_3) iD, k = min((int)s, nknots - 2),
 *     t = s - (T)k, g = g_k + t dg_k, G = G_k + t dG_k.  A partner that is in_3 with r2 < x0_3 has no value: g = G = NaN, the
 *     deliberate rule of a pair below the pair table.
 *   - Angular parameters.  lambda_host and cos0_host: ntypes^3 doubles each, [a][b][c] with a the centre; finite, exactly
 *     symmetric in (b, c), cos0 in [-1, 1]; rounded to T once.  ntypes <= NL_SW_MAX_TYPES.
 *   - Partners.  j and k range over the entries of row i of the list of the last build (the filtered list where an exclusion or
 *     type table is set) that are in_3: an excluded partner, or one of a pair of types with rc_ab = 0, forms no triple.
 *   - Per partner j of centre i, once: a = r_i - r_j from the image rule of nl_lj_forces, r2_a = ax ax + ay ay + az az as the
 *     pair function writes it; r = sqrt(r2_a), ir_a = 1 / r, ir2_a = ir_a ir_a, g_a and G_a from the slot (t_i, t_j).
 *   - Per ordered pair of partners (j, k), k != j, with b, ir_b, g_b of k, Lambda and c0 of (t_i, t_j, t_k), every product and
 *     sum below one operation in the order the brackets give:
 *       cs = (((ax bx + ay by) + az bz) ir_a) ir_b       dc = cs - c0       ld = Lambda dc       ldd = ld dc
 *       q = g_a g_b       h = ldd q       a2 = (ld + ld) q       cb = a2 (ir_a ir_b)       ca = ldd (G_a g_b) + a2 (cs ir2_a)
 *     The force on the end j from the triple is cb b - ca a, which is
 *       F_j = -Lambda dc^2 G_a g_b a + 2 Lambda dc g_a g_b (b ir_a ir_b - cs a ir_a^2).
 *     It is summed over k in parts: sa = sum_k ca, sb = sum_k (cb b) (per component), e_j = sum_k h, each a sum in T in no
 *     promised order; then F_j = sb - sa a, one product and one difference per component.  F_k is the same from k's side, and
 *     the centre receives F_i = -(sum_j F_j), the sum over its partners in T, negated.
 *   - f_dev is n x 4 of T: {fx, fy, fz, pe_i}.  It is zeroed by a kernel, then every centre i adds its own value
 *     {pair force of its row + F_i, half its pair energies + (sum_j e_j) (T)(1/6)} -- each of the two a sum in T as
 *     nl_table_forces forms it, then one addition -- and to each partner j {F_j, e_j (T)(1/3)}, by floating-point atomics.  So
 *     pe_i holds half the pair energies and a third of h for each particle of a triple (the LAMMPS per-atom convention):
 *     sum pe_i = E.
 *   - Totals, the 8 doubles of nl_lj_virial.  The pair part is nl_table_virial's, with in = in_phi || in_3 for n_in.  The
 *     three-body part adds, per centre i and partner j, W_cd -= a_c F_j,d for (c, d) = xx, yy, zz, xy, xz, yz -- the product
 *     in T from the F_j above, negated, converted -- and U += e_j / 2: every triple once (the kernel doubles the W term in
 *     double in front of the factor 1/2 of a full list, which is exact).  Summed in double in one fixed order.
 *   - Full lists only.  A row must hold all partners of its centre: after a NL_LIST_HALF build the four calls return
 *     NL_ERR_STATE.  Slab builds (local-index ones included) and distributed builds: NL_ERR_STATE -- the force on an owned end
 *     needs the triples centred on ghosts.
 *   - At most NL_SW_MAX_NEAR partners in_3 per centre.  A centre with more has no value: NaN in all four columns of the centre
 *     and of every partner of it that is in_3, and in all 8 totals.  A clamp would be silently wrong physics, and an error
 *     word would need a host sync.  Rows may be any length: only the in-range partners count.
 *   - NaN otherwise: where the arithmetic above gives it.  A partner below r_min_3 of a centre with at least two partners in_3
 *     makes the centre and all its in_3 partners NaN (all four columns) and all 8 totals; a centre with that one partner
 *     alone has no triple and no NaN.
 *   - Reproducibility.  The totals use no atomic and one fixed order: two nl_sw_virial calls on the same list and positions
 *     give the same 8 doubles, bit for bit.  The forces reach the ends, and the centres, by floating-point atomics: f_dev is
 *     reproducible only within the tested bound.
 *   - Types.  ntypes == 1: one slot, with or without a type table.  ntypes > 1 needs a type table of exactly that ntypes
 *     (NL_ERR_STATE without one, NL_ERR_ARG for another ntypes) and a pair table of 1 or ntypes types: nl_set_eam's rules.
 *   - Reach, at the calls: r_max of the pair table and r_max_3 <= rc for the synchronous calls, <= rc - skin for the enqueue
 *     calls; with a type table <= rc_ab (less the skin) for every rc_ab > 0.  Else NL_ERR_ARG.
 *   - nl_set_sw: 2 <= nknots <= NL_TABLE_MAX_KNOTS, 0 < r_min_3 < r_max_3, 1 <= ntypes <= NL_SW_MAX_TYPES, finite tables, angular
 *     parameters as above, else NL_ERR_ARG and the old tables are kept.  nknots == 0 or four NULL arrays clear the tables (some of
 *     them NULL: NL_ERR_ARG).  Synchronous; the device buffer is kept where the new tables fit; the list is not touched.
 *     nl_get_sw: the scalars, and lds: whether the forces and totals read their tables from LDS; NL_ERR_STATE while no tables
 *     are set.
 *   - Kernels.  The persistent grid of the table kernels, one wave per centre row: the row is walked once (pair part; the in_3
 *     partners compacted into a per-wave LDS strip of 64 x {j, a}), then every lane holds one partner and loops over all of
 *     them.  The pair table and the g tables are staged in LDS where together with the block's strips (4 x 64 x (3 sizeof(T)
 *     + 4) bytes) they fit NL_TABLE_LDS_BYTES, else both are read from global memory; NL_TABLE_LDS=0 in the environment of
 *     nl_set_sw forces the global path.  Both paths compute the same totals bit for bit.
 *   - Everything else (ordering, state, NaN on a non-zero status word, n == 0, the totals' scratch with its first-call rule, the
 *     enqueue variants copy nothing and can be captured) is nl_table_forces' / nl_table_virial's.
 * Tested contract (tests/test_sw.py): every component of every particle within SW_C u S and the totals
 * within SW_CW u S of an O(N m^2) float64 evaluation of the same rule (md_neighbor_list_amd.sw three_body), S the uncancelled
 * sums over pairs and triples including the conditioning of each table read on the rounding of its r2. */
#define NL_SW_MAX_TYPES 4
#define NL_SW_MAX_NEAR 64
int nl_set_sw(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min_3, double r_max_3, const double* g_host,
              const double* G_host, const double* lambda_host, const double* cos0_host);
int nl_get_sw(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min_3, double* r_max_3, int32_t* lds);
int nl_sw_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_sw_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_sw_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);
int nl_sw_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);

/* Tersoff-type bond-order potentials (LAMMPS pair_style tersoff, HOOMD md.many_body.Tersoff: silicon, germanium and carbon in
 * the Tersoff 1988/89 forms, SiC, SiGe, GaN, BN, the Albe-Erhart parametrisations): forces, per-particle energies and the 8
 * totals of
 *   E = sum_pairs phi(r) + sum_i sum_{j != i} 1/2 b(zeta_ij) u_{t_i t_j}(r_ij),
 *   zeta_ij = p_{t_i t_j}(r_ij) sum_{k != i, j} g_{t_i t_j t_k}(cos theta_jik) q_{t_i t_k}(r_ik),
 * j, k the partners of the centre i in the list.  For Tersoff the caller samples phi = f_C A exp(-lambda_1 r) into the pair
 * table, u = -f_C B exp(-lambda_2 r), q = f_C exp(-lambda_3 r), p = exp(lambda_3 r): the m = 1 form, whose exponential of
 * r_ij - r_ik factorises (md_neighbor_list_amd/tersoff.py samples them).  The rule, for both position types T, with one rounding
 * per operation, no contraction, and sqrt and / the correctly rounded IEEE operations:
 *   - Pair part.  phi is the handle's pair table (nl_set_pair_table), evaluated by exactly the rule stated there: fr_phi,
 *     pe_phi, in_phi.  It must be set (NL_ERR_STATE otherwise); a model without a pair part passes zeros.
 *   - Radial tables u, q, p.  The knot format and the grid rule of nl_set_sw's g tables, one grid r_min_3, r_max_3, nknots for
 *     all three: ntypes x ntypes slots each, slot a ntypes + b for centre type a and end type b (not necessarily symmetric).
 *     The caller passes u[slot][k] = u(r) and U[slot][k] = -u'(r) / r at r = sqrt(x_k), finite, and q, Q, p, P alike.  One knot
 *     index k and one t serve the three reads: v = v_k + t dv_k.  in_3 = r2 < xc_3 && r2 > 0; a partner that is in_3 with
 *     r2 < x0_3 has no value: u = U = q = Q = p = P = NaN.  p and P may both be NULL (lambda_3 = 0): then p = 1 and P = 0 by
 *     value and nothing is read (one of them NULL: NL_ERR_ARG).
 *   - Angular function.  gamma, c2_over_d2 = c^2 / d^2, d2 = d^2 and hh = h: ntypes^3 doubles each, [a][b][c] with a the centre;
 *     it need not be symmetric in (b, c).  The host forms gc = gamma c2_over_d2 in double; gamma, gc, d2, h are rounded to T
 *     once.  With x = h - cs, x2 = x x, den = d2 + x2:
 *       g = gamma + gc (x2 / den)          g' = dg/dcs = -((((gc + gc) d2) x) / (den den))
 *     This is gamma (1 + c^2/d^2 - c^2 / (d^2 + (h - cos theta)^2)) rearranged: silicon has c^2/d^2 = 3.8e7, and in fp32 the
 *     difference of two numbers of that size would leave g, which is of order 1, without a correct digit.
 *   - Bond order.  beta and nn = n: ntypes^2 doubles each, [a][b], centre and end.  The device holds beta, n and
 *     e2 = (T)(-1 / (2 n)), the quotient taken in double.  zeta <= 0: b = 1, b' = 0.  Otherwise (a NaN zeta included, which so
 *     propagates)
 *       t = beta zeta      tn = pow(t, n)      b = pow(1 + tn, e2)      b' = (((T)(-0.5) b) (tn / (1 + tn))) / zeta
 *     The two pow calls (powf in fp32) are the only operations of the rule that are not one correctly rounded IEEE operation:
 *     the tested bound assumes each within 2 ulp of the exact power (an assumption: DESIGN.md section 8y).
 *   - Partners.  j and k range over the entries of row i of the list of the last build (the filtered list where an exclusion or
 *     type table is set) that are in_3: an excluded partner, or one of a pair of types with rc_ab = 0, forms no bond and enters
 *     no zeta.
 *   - Per partner j of centre i, once: a = r_i - r_j from the image rule of nl_lj_forces, r2_a = ax ax + ay ay + az az;
 *     ir_a = 1 / sqrt(r2_a), ir2_a = ir_a ir_a; u_j, U_j, q_j, Q_j, p_j, P_j from the slot (t_i, t_j).
 *   - First pass, per ordered pair of partners (j, k), k != j, with b_vec, ir_b, q_k of k and the parameters of (t_i, t_j, t_k):
 *       cs = (((ax bx + ay by) + az bz) ir_a) ir_b       g_jk as above       S_j = sum_k g_jk q_k  (a sum in T, no promised order)
 *     Then zeta_j = p_j S_j, b_j and b'_j as above, e_j = b_j u_j, w_j = ((T)0.5 u_j) b'_j, wp_j = w_j p_j.
 *   - Second pass, per ordered pair (j, k), k != j, g'_jk from the parameters of (t_i, t_j, t_k), g_kj and g'_kj from those of
 *     (t_i, t_k, t_j), all at the same cs, every product and sum one operation in the order the brackets give:
 *       cc = (wp_j g'_jk) q_k + (wp_k g'_kj) q_j       cb = cc (ir_a ir_b)       ca = cc (cs ir2_a) + (wp_k g_kj) Q_j
 *     sa = sum_k ca, sb = sum_k (cb b_vec) (per component), sums in T in no promised order; then
 *       rad = ((T)0.5 b_j) U_j + (w_j P_j) S_j       sat = sa + rad       F_j = sb - sat a
 *     one product and one difference per component.  This is the force on the end j from the bonds of the centre i,
 *       F_j = -(1/2 b_j U_j + w_j P_j S_j) a + sum_k [(w_j p_j g'_jk q_k + w_k p_k g'_kj q_j)(b_vec ir_a ir_b - cs a ir2_a) - w_k p_k g_kj Q_j a],
 *     and the centre receives F_i = -(sum_j F_j), the sum over its partners in T, negated.
 *   - f_dev is n x 4 of T: {fx, fy, fz, pe_i}.  It is zeroed by a kernel, then every centre i adds its own value {pair force of
 *     its row + F_i, half its pair energies + (sum_j e_j) (T)0.25} -- each of the two a sum in T as nl_table_forces forms it,
 *     then one addition -- and to each partner j {F_j, e_j (T)0.25}, by floating-point atomics.  So pe_i holds half the pair
 *     energies and a quarter of e_j for each end of every ordered bond (the LAMMPS per-atom convention): sum pe_i = E.
 *   - Totals, the 8 doubles of nl_lj_virial.  The pair part is nl_table_virial's, with in = in_phi || in_3 for n_in.  The bond
 *     part adds, per centre i and partner j, W_cd -= a_c F_j,d for (c, d) = xx, yy, zz, xy, xz, yz -- the product in T, negated,
 *     converted -- and U += e_j / 2, each ordered bond once (the kernel hands 2 x the W term and e_j, both exact in double, to
 *     the factor 1/2 of a full list).  Summed in double in one fixed order, no atomic.
 *   - Full lists only: after a NL_LIST_HALF build the four calls return NL_ERR_STATE.  Slab builds (local-index ones included)
 *     and distributed builds: NL_ERR_STATE.
 *   - At most NL_TERSOFF_MAX_NEAR partners in_3 per centre.  A centre with more has no value: NaN in all four columns of the
 *     centre and of every partner of it that is in_3, and in all 8 totals.
 *   - NaN otherwise: where the arithmetic above gives it.  A partner below r_min_3 makes the centre and all its in_3 partners
 *     NaN (all four columns) and all 8 totals.  Unlike Stillinger-Weber a centre with a single partner still has a bond
 *     (zeta = 0, b = 1), so a lone partner below r_min_3 is NaN too.
 *   - Reproducibility.  The totals use no atomic and one fixed order: two nl_tersoff_virial calls on the same list and positions
 *     give the same 8 doubles, bit for bit.  f_dev is reproducible only within the tested bound.
 *   - Types, reach: nl_set_sw's rules, with ntypes <= NL_TERSOFF_MAX_TYPES.
 *   - nl_set_tersoff: 2 <= nknots <= NL_TABLE_MAX_KNOTS, 0 < r_min_3 < r_max_3, 1 <= ntypes <= NL_TERSOFF_MAX_TYPES, every value
 *     finite, d2 > 0, beta >= 0, n > 0, else NL_ERR_ARG and the old state is kept.  nknots == 0 or all arrays NULL clear it.
 *     Synchronous; the device buffer is kept where the new tables fit; the list is not touched.  nl_get_tersoff: the scalars,
 *     has_p: whether p is set, and lds: whether the forces and totals read their tables from LDS; NL_ERR_STATE while nothing
 *     is set.
 *   - Kernels.  The persistent grid of the table kernels, one wave per centre row, nl_sw_forces' walk and strip; then two
 *     loops over the partners, the bond order between them.  The pair table and the radial tables are staged in LDS where
 *     together with the block's copy of the parameters ((ntypes^3 + ntypes^2) x 4 sizeof(T) bytes, always in LDS) and strips
 *     they fit NL_TABLE_LDS_BYTES, else both are read from global memory; NL_TABLE_LDS=0 in the environment of nl_set_tersoff
 *     forces the global path.  Both paths compute the same totals bit for bit.
 *   - Everything else (ordering, state, NaN on a non-zero status word, n == 0, the totals' scratch with its first-call rule, the
 *     enqueue variants copy nothing and can be captured) is nl_table_forces' / nl_table_virial's.
 * Out of scope: m = 3 with lambda_3 != 0, slab and distributed lists, more than 64 partners, the Tersoff-ZBL and tersoff/mod forms.
 * Tested contract (tests/test_tersoff.py): every component of every particle within TERSOFF_C u S and the
 * totals within TERSOFF_CW u S of an O(N m^2) float64 evaluation of the same rule (md_neighbor_list_amd.tersoff bond_energy), S
 * the uncancelled sums including the conditioning of each table read on its r2 and of b and b' on zeta. */
#define NL_TERSOFF_MAX_TYPES 4
#define NL_TERSOFF_MAX_NEAR 64
int nl_set_tersoff(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min_3, double r_max_3, const double* u_host,
                   const double* U_host, const double* q_host, const double* Q_host, const double* p_host, const double* P_host,
                   const double* gamma_host, const double* c2_over_d2_host, const double* d2_host, const double* h_host,
                   const double* beta_host, const double* n_host);
int nl_get_tersoff(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min_3, double* r_max_3, int32_t* has_p, int32_t* lds);
int nl_tersoff_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_tersoff_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, void* f_dev, void* stream);
int nl_tersoff_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);
int nl_tersoff_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double* out_dev, void* stream);

/* Per-particle charges: forces, per-particle energies and the 8 totals of E = sum_pairs [ phi_{t_i t_j}(r) + q_i q_j C(r) ]
 * over the entries of the list of the last build (the filtered list where an exclusion or type table is set).  C(r) is any
 * short-range electrostatic pair term the caller has sampled: the real-space part of Ewald / PME erfc(alpha r) / r, damped
 * shifted force, Wolf, reaction field, Debye-Hueckel (md_neighbor_list_amd/coulomb.py samples them).  A pair table has one
 * slot per pair of types, so it cannot carry a charge per particle; this consumer can.  The rule, both position types T, one
 * rounding per operation, no contraction:
 *   - Pair part.  phi is the handle's pair table (nl_set_pair_table), evaluated by exactly the rule stated there, slots and
 *     all: fr_phi, pe_phi, in_phi.  It must be set (NL_ERR_STATE otherwise); a model without a pair part passes zeros, as for
 *     nl_set_eam.
 *   - Charge table.  One slot on a grid of its own, with the grid rule of nl_set_pair_table: D = (r_max_c^2 - r_min_c^2) /
 *     (nknots - 1), x_k = r_min_c^2 + k D.  The caller passes C[k] = C(r) and K[k] = -C'(r) / r at r = sqrt(x_k), nknots
 *     doubles each, finite; the Coulomb constant and the dielectric are folded in by the caller.  Device form: the knot
 *     {K_k, dK_k, C_k, dC_k} in T, differences taken in double and rounded once, 0 at the last knot; x0_c = (T)(r_min_c^2),
 *     xc_c = (T)(r_max_c^2), iD = (T)(1 / D).
 *   - Charges.  charge_dev holds one T per row of q_dev, in its order; after a local-index slab build these are the n
 *     positions of the build, ghosts included (the ghosts' charges arrive with the caller's halo, as their positions do).  It
 *     is read, never copied, and is the caller's to keep valid; a caller who re-sorts permutes it with nl_resort like any
 *     other array.  NULL: NL_ERR_ARG.  A NaN or infinite charge propagates by the arithmetic; nothing validates charges
 *     (that would need a sync).
 *   - Per entry (row i, partner j): d from the image rule of nl_lj_forces; r2 = dx dx + dy dy + dz dz as the pair table's
 *     pair function writes it; qq = q_i q_j; in_c = r2 < xc_c && r2 > 0; s = (r2 - x0_c) iD, k = min((int)s, nknots - 2),
 *     t = s - (T)k.  Where in_c: kc = K_k + t dK_k, cc = C_k + t dC_k, fc = qq kc, ec = qq cc; otherwise both are 0.  A pair
 *     that is in_c with r2 < x0_c has no value: fc and ec are NaN whatever the charges (two neutral particles included), by
 *     the deliberate rule of a pair below the pair table.  fr = fr_phi + fc, pe = pe_phi + ec, (fx, fy, fz) = fr d, the force
 *     on i; in = in_phi || in_c.
 *   - Everything else is nl_table_forces / nl_table_virial: the layouts of f_dev (n_rows x 4 of T: fx, fy, fz, pe_i) and
 *     out_dev (8 doubles, n_in the pairs with `in`), the half list's reaction by atomics after zeroing and full rows written
 *     once, the factor 1/2 of a full list in the totals, the ghost rules of local-index slab lists, which are accepted (there
 *     only a one-type pair table is reachable), NaN on a non-zero status word, n == 0, the shared scratch of the totals with
 *     its first-call rule, totals reproducible bit for bit, enqueue variants that copy nothing and can be captured, and
 *     NL_ERR_STATE after a distributed build or a slab build made without nl_set_local_ids.
 *   - Reach, at the calls: r_max of the pair table and r_max_c <= rc for the synchronous calls, <= rc - skin for the enqueue
 *     calls; with a type table <= rc_ab (less the skin) for every rc_ab > 0.  Else NL_ERR_ARG.  A pair of types with
 *     rc_ab = 0 has no entries and therefore no charge term either: a model whose charged types must always interact gives
 *     every pair of them a cut-off.
 *   - nl_set_coulomb_table: 2 <= nknots <= NL_TABLE_MAX_KNOTS, 0 < r_min < r_max, finite values, `which` == NL_COUL_LIST,
 *     else NL_ERR_ARG and the old table is kept.  nknots == 0, or K_host and C_host both NULL, clears the table (one of them
 *     alone NULL is NL_ERR_ARG).  Synchronous; the device buffer is kept where the new table fits; the list is not touched.
 *     nl_get_coulomb_table: the scalars and whether the calls read both tables from LDS; NL_ERR_STATE while no table is set.
 *     `which` names the table: NL_COUL_LIST is the term over the list; every other value is NL_ERR_ARG (the term over the
 *     pairs that nl_set_exclusions removed, Ewald's correction for bonded pairs, has a table and entry points of its own:
 *     nl_set_coul_excl_table below).
 *   - Kernels.  The persistent grid of the table kernels.  The pair table and the charge table both in LDS where together
 *     they fit NL_TABLE_LDS_BYTES, else both from global memory.  NL_TABLE_LDS=0 in the environment of nl_set_coulomb_table
 *     forces the global path.  Both paths compute the same bits.
 * Tested contract (tests/test_coulomb.py): every component of every particle within COUL_C u S and the
 * totals within COUL_CW u S of an O(N^2) float64 evaluation of the same rule, S the uncancelled sums including the
 * conditioning of s on the rounding of r2 for both tables. */
enum { NL_COUL_LIST = 0 };
int nl_set_coulomb_table(nl_handle_t h, int which, int32_t nknots, double r_min, double r_max, const double* K_host,
                         const double* C_host);
int nl_get_coulomb_table(nl_handle_t h, int which, int32_t* nknots, double* r_min, double* r_max, int32_t* lds);
int nl_coul_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, void* stream);
int nl_coul_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, void* stream);
int nl_coul_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev, void* stream);
int nl_coul_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev,
                           void* stream);

/* The excluded-pair term of the charges: forces, per-particle energies and the 8 totals of E = sum q_i q_j C(r) over the
 * pairs of the handle's exclusion table.  nl_set_exclusions takes the bonded pairs out of the list, but the reciprocal sum of
 * Ewald / PME still contains them, so the real-space side owes -q_i q_j erf(alpha r) / r for each of them
 * (md_neighbor_list_amd/coulomb.py ewald_excluded samples it; ewald_self is the self-energy).  nl_coul_forces followed by
 * nl_coul_excl_forces with `add` on the same stream leaves the complete real-space force in one buffer.  The rule, both
 * position types T, one rounding per operation, no contraction:
 *   - Table.  One slot on a grid of its own, with the grid rule and the device form of nl_set_coulomb_table: the knot
 *     {K_k, dK_k, C_k, dC_k} in T with C[k] = C(r), K[k] = -C'(r) / r at r = sqrt(x_k); x0 = (T)(r_min^2), xc = (T)(r_max^2),
 *     iD = (T)(1 / D).  The sign belongs to the table (Ewald's is C = -prefactor erf(alpha r) / r).  No pair table is needed:
 *     this term has no phi.
 *   - Entries.  The sum runs over the handle's exclusion table as it is at the call: the symmetric, sorted, deduplicated CSR
 *     of nl_get_exclusions, after any relabelling by nl_resort.  Row i holds each partner j once, and row j holds i.
 *   - Per entry (row i, partner j): d = r_i - r_j from the image rule of nl_lj_forces with the box and mask of the last build
 *     (folded with rint in z, y, x order with the tilts): the nearest image, which does not depend on the list -- the pairs are
 *     not in it.  r2 = dx dx + dy dy + dz dz as nl_coul_forces writes it; qq = q_i q_j; s = (r2 - x0) iD,
 *     k = min((int)s, nknots - 2), t = s - (T)k; fc = qq (K_k + t dK_k), ec = qq (C_k + t dC_k); the force on i is fc d.
 *   - No cut-off.  An excluded pair is owed its term wherever it is, and the calls do not test any reach against rc or the
 *     skin.  A pair with !(r2 >= x0 && r2 < xc) -- r2 == 0 and a NaN r2 included -- is NaN in fc and ec whatever the charges:
 *     the deliberate rule of a pair below the pair table (a zero would be silently wrong physics).
 *   - Forces.  f_dev is n x 4 of T, {fx, fy, fz, pe_i}, pe_i half the row's ec.  Every row is produced by one group of 8 lanes
 *     and stored once.  add == 0: the row's four values are written (an empty row: zeros).  add != 0: they are added to what
 *     f_dev holds, by one plain read-modify-write per row and no atomic.  The sums have one fixed order: lane g of the group
 *     its entries g, g + 8, ... of the row, then the lanes g and g ^ 4, ^ 2, ^ 1; two calls give the same bits.
 *   - Totals.  The 8 doubles of nl_lj_virial, every entry weighted 1/2 (exact), terms formed in T, converted and summed in
 *     double in one fixed order; n_in is the number of distinct excluded pairs.  Any NaN entry makes all 8 values NaN.  They
 *     use the scratch of nl_lj_virial with its first-call rule.
 *   - State and ordering: those of nl_coul_forces / nl_coul_forces_enqueue, and: the last build must be a whole single-device
 *     build whose ids are its rows -- slab builds (local-index ones included) and distributed builds are NL_ERR_STATE; no
 *     exclusion table, or no table of this term: NL_ERR_STATE; an exclusion table whose n differs from the build's n (a global
 *     table with n_ids > n, the only way to get there): NL_ERR_ARG; charge_dev == NULL: NL_ERR_ARG.  n == 0 (looked at before
 *     the table's n): nothing is written and the totals are 8 zeros.  A non-zero status word in the enqueue variants: NaN rows
 *     (with `add` as well) and 8 NaN totals.  The enqueue variants copy nothing from the host and can be captured; a caller
 *     who captured them captures again after nl_set_exclusions*, which may move the table.
 *   - nl_set_coul_excl_table: the arguments, the clearing rule and the buffer rule of nl_set_coulomb_table; NL_TABLE_LDS=0 in
 *     its environment forces the global path.  nl_get_coul_excl_table: the scalars and whether the calls read the table from
 *     LDS (it fits NL_TABLE_LDS_BYTES); NL_ERR_STATE while no table is set.
 *   - Kernels.  A wave takes 8 consecutive rows, 8 lanes per row; blocks of 256 threads (32 rows) on persistent grids, the
 *     totals' of min(ceil(n / 32), NL_COUL_EXCL_BLOCKS) blocks, each of which leaves one partial of 8 doubles.  Both table
 *     paths compute the same bits.
 * Tested contract (tests/test_coul_excl.py): every component of every particle within COULX_C u S and
 * the totals within COULX_CW u S of a float64 loop over the table's pairs. */
#define NL_COUL_EXCL_BLOCKS 256 /* most blocks of the totals of the excluded-pair term */
int nl_set_coul_excl_table(nl_handle_t h, int32_t nknots, double r_min, double r_max, const double* K_host, const double* C_host);
int nl_get_coul_excl_table(nl_handle_t h, int32_t* nknots, double* r_min, double* r_max, int32_t* lds);
int nl_coul_excl_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, int add,
                        void* stream);
int nl_coul_excl_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, void* f_dev, int add,
                                void* stream);
int nl_coul_excl_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev, void* stream);
int nl_coul_excl_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* charge_dev, double* out_dev,
                                void* stream);

/* The DPD pair thermostat: forces, per-particle energies and the 8 totals of
 *   F_ij = -phi'(r) e_ij + [ -gamma w(r)^2 (e_ij . v_ij) + sigma w(r) xi_ij / sqrt(dt) ] e_ij
 * over the entries of the list of the last build (LAMMPS pair_style dpd and dpd/tstat, HOOMD md.pair.DPD): dissipative
 * particle dynamics proper where phi is a soft conservative table (md_neighbor_list_amd/dpd.py samples it), and the
 * momentum-conserving, Galilean-invariant thermostat of any other tabulated potential.  The rule, both position types T, one
 * rounding per operation, no contraction:
 *   - Pair part.  phi is the handle's pair table (nl_set_pair_table), evaluated by exactly the rule stated there: fr_phi,
 *     pe_phi, in_phi.  It must be set (NL_ERR_STATE otherwise); a pure thermostat passes zeros, as for nl_set_eam.
 *   - Weight table.  One slot on a grid of its own, with the grid rule of nl_set_pair_table: D = (r_max^2 - r_min^2) /
 *     (nknots - 1), x_k = r_min^2 + k D.  The caller passes A[k] = w(r) / r at r = sqrt(x_k), nknots finite doubles.  Device
 *     form: the knot {A_k, dA_k, 0, 0} in T, dA_k = (T)(A[k+1] - A[k]), 0 at the last knot; x0_d = (T)(r_min^2), xc_d =
 *     (T)(r_max^2), iD = (T)(1 / D).  No square root per pair: w e = (w / r) d and w^2 (e . v) e = (w / r)^2 (d . v) d; the
 *     dissipative weight is the square of the interpolated A, so w_D = w_R^2 holds exactly, as the fluctuation-dissipation
 *     relation asks.
 *   - Parameters.  gamma_host and sigma_host: nslots = ntypes (ntypes + 1) / 2 doubles each, at slot(a, b) of
 *     nl_pair_histogram_typed, finite and >= 0; dt > 0 and finite.  The device holds g = (T)gamma and sg = (T)(sigma /
 *     sqrt(dt)) per slot, the quotient taken in double and rounded once.  sigma = sqrt(2 gamma kT) is the caller's choice
 *     (dpd.sigma_for); sigma = 0 is pure friction.  ntypes = 1 works with or without a type table; ntypes > 1 needs a type
 *     table of exactly that ntypes (NL_ERR_STATE without one, NL_ERR_ARG for another ntypes) and a pair table of 1 or ntypes
 *     types: nl_set_eam's rules.
 *   - Pair noise.  Integers only, the same for both T, all arithmetic modulo 2^64.  fin(z): z ^= z >> 30; z *=
 *     0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.  Per call key = fin(fin(seed) + step), step =
 *     *step_dev, read on the device by the kernel and never by the host.  Per entry (row i, partner j): lo = min(i, j), hi =
 *     max(i, j) as unsigned 32-bit values, z = fin(key + ((uint64)lo << 32 | hi)), m = z >> 40 (24 bits), xi = (T)(2 m + 1 -
 *     2^24) (T)(sqrt(3) / 2^24).  The integer is odd and below 2^24 in magnitude: exact in fp32, never 0, symmetric about 0;
 *     xi is uniform with unit variance, which is sufficient for DPD (Groot & Warren 1997), and is the same number from both
 *     rows of a full list, from a half list, in fp32 and in fp64.
 *   - Per entry: d from the image rule of nl_lj_forces; r2 = dx dx + dy dy + dz dz as the pair table's pair function writes
 *     it; in_d = r2 < xc_d && r2 > 0; s = (r2 - x0_d) iD, k = min((int)s, nknots - 2), t = s - (T)k, A = A_k + t dA_k;
 *     dv = v_i - v_j per component, dot = (dx dvx + dy dvy) + dz dvz; fd = -((g (A A)) dot), fn = (sg A) xi; f_dpd = in_d ?
 *     fd + fn : 0, selected, not multiplied.  fr = fr_phi + f_dpd, pe = pe_phi, (fx, fy, fz) = fr d, the force on i; in =
 *     in_phi || in_d.  A pair that is in_d with r2 < x0_d has no value: fr and pe are NaN whatever gamma and sigma, by the
 *     deliberate rule of a pair below the pair table.
 *   - Symmetry.  The image and a - b are odd under the swap of the two particles; dot, r2, A and xi are even.  So after a full
 *     build the two rows of a pair compute the same fr, bit for bit, and exactly opposite forces; the sums of the rows differ
 *     only by their order.
 *   - Arguments.  v_dev: n rows in the position type, v_stride 3 or 4, read and never copied.  step_dev: one 64-bit device
 *     word, the caller's, which the caller advances in stream order (a captured step that increments it draws fresh noise at
 *     every replay).  NULL for either, or another v_stride: NL_ERR_ARG.
 *   - Everything else is nl_coul_forces / nl_coul_virial: the layouts of f_dev (n x 4 of T) and out_dev (8 doubles: W from
 *     the whole fr, U = sum pe_phi, n_in the pairs with `in`), the half list's reaction by atomics after zeroing and full rows
 *     written once, the factor 1/2 of a full list, NaN on a non-zero status word, n == 0, the shared scratch of the totals
 *     with its first-call rule, enqueue variants that copy nothing and can be captured.  The totals are reproducible bit for
 *     bit for the same positions, velocities and step.
 *   - Reach, at the calls: r_max of both tables <= rc, <= rc - skin for the enqueue calls; with a type table <= rc_ab (less
 *     the skin) for every rc_ab > 0.  Else NL_ERR_ARG.
 *   - Lists served: whole single-device builds whose ids are their rows, half and full.  Lists of caller ids, distributed
 *     builds and every slab build, local-index ones included, are NL_ERR_STATE: a crossing pair would be keyed by two different
 *     local row pairs on its two ranks, and momentum conservation would be lost.  After nl_resort (positions and velocities
 *     permuted alike) the rows, and hence the noise assigned to a physical pair, change; the statistics do not.
 *   - nl_set_dpd: 2 <= nknots <= NL_TABLE_MAX_KNOTS, 0 < r_min < r_max, 1 <= ntypes <= NL_MAX_TYPES, values as above, else
 *     NL_ERR_ARG and the old state is kept.  nknots == 0, or the three arrays all NULL, clears the state (some of them NULL
 *     is NL_ERR_ARG).  Synchronous; the device buffer is kept where the new state fits, so a captured graph then reads a
 *     changed gamma, sigma, dt or seed; the list is not touched.  nl_get_dpd: the scalars and whether the calls read their
 *     tables from LDS; NL_ERR_STATE while nothing is set.
 *   - Kernels.  The persistent grid of the table kernels.  The pair table, the weight table and the slot parameters in LDS
 *     where together they fit NL_TABLE_LDS_BYTES, else all from global memory.  NL_TABLE_LDS=0 in the environment of
 *     nl_set_dpd forces the global path.  Both paths compute the same bits.  The key is computed once per wave.
 * Tested contract (tests/test_dpd.py): every component of every particle within DPD_C u S and the totals
 * within DPD_CW u S of an O(N^2) float64 evaluation of the same rule, S the uncancelled sums including the conditioning of
 * both table reads on the rounding of r2 and of dot on the rounding of dv; the integer m itself, recovered from the forces of
 * isolated dimers. */
int nl_set_dpd(nl_handle_t h, int32_t ntypes, int32_t nknots, double r_min, double r_max, const double* A_host,
               const double* gamma_host, const double* sigma_host, double dt, uint64_t seed);
int nl_get_dpd(nl_handle_t h, int32_t* ntypes, int32_t* nknots, double* r_min, double* r_max, double* dt, uint64_t* seed,
               int32_t* lds);
int nl_dpd_forces(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride,
                  const uint64_t* step_dev, void* f_dev, void* stream);
int nl_dpd_forces_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride,
                          const uint64_t* step_dev, void* f_dev, void* stream);
int nl_dpd_virial(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride,
                  const uint64_t* step_dev, double* out_dev, void* stream);
int nl_dpd_virial_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, const void* v_dev, int32_t v_stride,
                          const uint64_t* step_dev, double* out_dev, void* stream);

/* The pair-distance histogram of the list, the counts behind a radial distribution function g(r): for everybody
 * (nl_pair_histogram) or per unordered pair of types (nl_pair_histogram_typed).  The rule:
 *   - Entries.  The sum runs over the entries (row i, partner j) of the list of the last build: the filtered list where an
 *     exclusion or type table is set.  After a NL_LIST_HALF build every entry counts, after a NL_LIST_FULL build only the
 *     entries with j > i: both kinds count every stored pair once, in the row of the smaller id, and a half and a full
 *     build of the same input give the same counters, bit for bit.
 *   - Distance.  d = r_i - r_j at the image of nl_lj_forces (lj_image: folded on the periodic axes of the build's mask in z,
 *     y, x order with the tilts; positions up to one box length outside the box).  r2 = (dx dx + dy dy) + dz dz in the
 *     position type T, without FMA.
 *   - Bins, uniform in r.  In double e_k = (k r_max) / nbins for k = 0 .. nbins, and E_k is the largest T <= e_k e_k (the
 *     rounding of the builds' rc^2 and of the type table's thresholds); E_0 = 0.  An entry falls into bin b iff
 *     E_b <= r2 < E_{b+1}.  r2 >= E_nbins is counted nowhere, and neither is a NaN r2 (the call returns all the same).
 *     A coincident pair (r2 == 0) falls into bin 0 -- unlike the Lennard-Jones calls, whose pair function leaves r2 == 0 out.
 *   - Output.  hist_dev: nslots x nbins uint64_t on the device, row-major, for both position types.  The call ADDS to it:
 *     the caller zeroes it and owns it, so many frames accumulate.  Untyped: nslots = 1.  Typed: nslots = ntypes (ntypes +
 *     1) / 2 and an entry goes to slot(a, b) = a (2 ntypes - a + 1) / 2 + (b - a), a = min(t_i, t_j), b = max(t_i, t_j),
 *     the types those of nl_set_type_cutoffs.  No Lennard-Jones parameters are needed.
 *   - Reach.  r_max > 0 and finite, 1 <= nbins <= NL_HIST_MAX_BINS, else NL_ERR_ARG.  Untyped: r_max <= rc, and with a
 *     type table r_max <= min_ab rc_ab (a table with some rc_ab = 0 therefore refuses the untyped call: NL_ERR_ARG).  Typed:
 *     NL_ERR_STATE without a type table; r_max <= rc_ab for every pair of types with rc_ab > 0; a pair with rc_ab = 0 has
 *     no entries and its slot stays as it was.  The enqueue variants: the same limits less the skin, as
 *     nl_lj_forces_enqueue.
 *   - Ordering and state: those of nl_lj_forces and nl_lj_forces_enqueue, checks in the same order; slab and distributed
 *     builds are NL_ERR_STATE (but for a local-index slab list, below); n == 0 adds nothing.  Where an enqueue variant finds a non-zero status word it adds
 *     nothing; the error itself surfaces at the next nl_synchronize.
 *   - Capture.  The enqueue variants copy nothing from the host and no call ever allocates (every block computes the
 *     edges itself, into LDS): they can be captured from the first call on.
 *   - Exact and reproducible.  Integer counters only, 64 bits wide in LDS and in hist_dev: none can wrap for any list the
 *     library can build, 64-bit offsets included.  Two calls on the same list and positions add the same values.
 *   - One wave per row over a grid of at most 2048 blocks of 4 waves.  Where nslots x nbins <= NL_HIST_LDS_COUNTERS a block
 *     counts in LDS and adds its non-zero counters to hist_dev at its end; a larger histogram is added to hist_dev entry
 *     by entry.  Both give the same counters.
 *   - On a local-index slab list (nl_set_local_ids) the rows are the n_rows owned particles and the counters keep their
 *     unit of whole pairs.  Per entry (row i owned, partner j; j is a ghost iff j >= n_rows): an owned partner counts as
 *     above (half: every entry; full: j > i); a ghost partner counts iff dz < 0, or dz == 0 and z_i < z_j as raw
 *     coordinates, d = r_i - r_j the image above.  That image is exactly antisymmetric under the swap of the two particles
 *     and r2 is symmetric, so exactly one of the two ranks that store a crossing pair counts it, in the same bin: the
 *     counters of the ranks add up, bit for bit, to those of the whole-box call, and a half and a full slab build give the
 *     same counters.
 * Tested contract (tests/test_pair_histogram.py): equal, bin by bin, to an O(N^2) float64 count that
 * uses no list wherever no pair lies within 2^-17 (fp32; 2^-46 fp64; relative, r^2) of an edge; elsewhere the cumulative
 * counts are bracketed by the pairs surely below each edge and those within its band. */
#define NL_HIST_MAX_BINS 4096
#define NL_HIST_LDS_COUNTERS 4096
int nl_pair_histogram(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins, uint64_t* hist_dev,
                      void* stream);
int nl_pair_histogram_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins,
                              uint64_t* hist_dev, void* stream);
int nl_pair_histogram_typed(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins, uint64_t* hist_dev,
                            void* stream);
int nl_pair_histogram_typed_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, int32_t nbins,
                                    uint64_t* hist_dev, void* stream);

/* Steinhardt bond-orientational order parameters of every particle, from the list: q_l, the normalised third-order invariant
 * w_l and their neighbour-averaged forms (Lechner and Dellago), for one degree l per call.  The rule:
 *   - Neighbours.  The neighbours of a centre i are the entries j of row i of the list of the last build with 0 < r2 < X: the
 *     filtered list where an exclusion or type table is set, so an excluded partner is no neighbour, and neither is a partner
 *     of a type pair with rc_ab = 0 (the supported way to an order parameter over chosen species: give the pairs of types
 *     that shall not count rc_ab = 0).  d = r_i - r_j at the image of nl_lj_forces (lj_image), r2 = (dx dx + dy dy) + dz dz in
 *     the position type T, without FMA; X is the largest T <= r_max r_max taken in double (the rounding of the histogram's
 *     edges).  N_b(i) is their number.
 *   - The bond.  ir = 1 / sqrt(r2); u = (x, y, z) = ((-dx) ir, (-dy) ir, (-dz) ir), the unit vector from i to j.
 *   - Y_lm(u) for m = 0 .. l, complex with the Condon-Shortley phase (scipy's sph_harm), without a trigonometric function:
 *       c_0 = 1,  c_m = c_{m-1} (x + i y):  re' = re x - im y,  im' = re y + im x                     ((x + i y)^m)
 *       P_m = S_m,  P_k = (A_km z) P_{k-1} - B_km P_{k-2}  for k = m + 1 .. l  (P_{m-1} = 0)          (degree recurrence)
 *       Y_lm = (P_l re(c_m), P_l im(c_m))
 *     with  A_km = sqrt((4 k^2 - 1) / (k^2 - m^2)),  B_km = A_km sqrt(((k - 1)^2 - m^2) / (4 (k - 1)^2 - 1))  and
 *     S_m = (-1)^m sqrt((2 m + 1) / (4 pi) prod_{i = 1 .. m} (2 i - 1) / (2 i)),  formed in double on the host and rounded to T
 *     once.  Every operation is + - x or a correctly rounded sqrt or division, one rounding each.  A bond along z (x = y = 0)
 *     needs no special case: c_m = 0 exactly for m > 0.
 *   - q_lm(i) = (sum over the neighbours of Y_lm) / (T)N_b, the sum taken lane by lane along the row and then across the
 *     wave's lanes, real and imaginary part apart.  m < 0 follows from q_{l,-m} = (-1)^m conj(q_lm) and is not stored.
 *   - s = |q_l0|^2 + 2 sum_{m>0} |q_lm|^2 (|q|^2 = re re + im im);  q_l = sqrt(c s) with c = 4 pi / (2 l + 1) rounded to T.
 *   - w_l = (sum over m1, m2 = -l .. l with |m1 + m2| <= l of W[m1][m2] Re((q_lm1 q_lm2) q_lm3), m3 = -m1 - m2) / (s sqrt(s)),
 *     (a b) = (a_r b_r - a_i b_i, a_r b_i + a_i b_r) and Re(p c) = p_r c_r - p_i c_i, W the caller's 3j table rounded to T.  Where
 *     s = 0 (q_l = 0: an odd l at a centre of inversion) w_l is 0 / 0 = NaN.
 *   - With average != 0:  qa_lm(i) = (q_lm(i) + sum over the neighbours k of q_lm(k)) / (T)(N_b(i) + 1), the sum as above and
 *     taken first, over the same neighbours; the averaged q_l and w_l come from qa_lm by the same two formulas.
 *   - NaN rule.  A centre with N_b = 0 has no value: NaN in all four columns and in its q_lm (0 / 0).  A particle without
 *     neighbours is nobody's neighbour, so nothing spreads.  No clamp and no error word.
 * nl_set_steinhardt: 1 <= l <= NL_STEIN_MAX_L, r_max > 0 and finite; w3j_host: (2 l + 1)^2 finite doubles,
 * [m1 + l][m2 + l] = (l l l; m1 m2 -m1-m2) and 0 where |m1 + m2| > l, or NULL: no w_l, its columns are NaN.  Anything else is
 * NL_ERR_ARG and keeps the old setting; l == 0 clears it.  Synchronous: the tables are rounded to T once and uploaded.  The
 * list is not touched and nothing of a build changes: the next nl_update_list does not build because of it.
 * nl_steinhardt / nl_steinhardt_enqueue: out_dev is n x 4 of T, {q_l, w_l, averaged q_l, averaged w_l}; with average == 0
 * columns 2 and 3 are written as NaN ("not computed"), not left as they were.
 *   - Lists served: NL_LIST_FULL lists of whole single-device builds.  A row must hold every neighbour of its centre, for its
 *     own sum and again for the average, which needs q_lm of every partner.  A NL_LIST_HALF build, a slab build (a local-index
 *     one included: the average needs the ghosts' q_lm) and a distributed build are NL_ERR_STATE, and so is a call without a
 *     setting.
 *   - Reach.  r_max <= rc, and with a type table r_max <= rc_ab for every pair of types with rc_ab > 0; the enqueue variant:
 *     the same less the skin.  Else NL_ERR_ARG.
 *   - Scratch: q_lm and N_b of every row, sized by n_max and l, allocated by the first call (NL_ERR_STATE inside a capture: make
 *     one call before); allocated anew by the first call after an nl_initialize with another n_max or a setting with a
 *     larger l than any before.
 *   - Ordering, state, n == 0 (nothing is written) and capture: those of nl_table_forces and nl_table_forces_enqueue.  The
 *     enqueue variant copies nothing from the host; where it finds a non-zero status word it writes NaN to all four columns
 *     and to q_lm, and the error itself surfaces at the next nl_synchronize.
 *   - Reproducible.  No kernel uses an atomic: two calls on the same list and positions write the same bytes to out_dev and
 *     q_lm.  The order of a row's partners differs from build to build, so across builds only the tested bound holds.
 * nl_steinhardt_get_qlm: the un-averaged q_lm of the last call, [n][l + 1][2] of T (m = 0 .. l, {re, im}), and N_b as int32 [n];
 * l is that call's.  NL_ERR_STATE before a call.  Valid until the next call, setting with a larger l or nl_initialize.
 * Tested contract (tests/test_steinhardt.py): N_b exact and every value within STEIN_C u S of an O(N^2)
 * float64 evaluation with scipy-convention harmonics, S a first-order propagation of the roundings. */
#define NL_STEIN_MAX_L 12
int nl_set_steinhardt(nl_handle_t h, int32_t l, double r_max, const double* w3j_host);
int nl_get_steinhardt(nl_handle_t h, int32_t* l, double* r_max, int32_t* has_w);
int nl_steinhardt(nl_handle_t h, const void* q_dev, int32_t q_stride, int average, void* out_dev, void* stream);
int nl_steinhardt_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, int average, void* out_dev, void* stream);
int nl_steinhardt_get_qlm(nl_handle_t h, const void** qlm_dev, const int32_t** count_dev, int32_t* n, int32_t* l);

/* Clusters from the list: the connected components of the graph whose vertices are the member particles and whose edges are the
 * stored pairs within r_max (nl_clusters), and the count of solid-like bonds per particle after ten Wolde, Ruiz-Montero and
 * Frenkel (nl_solid_bonds), which turns the q_lm of nl_steinhardt into a member array.  The pipeline of a nucleation analysis:
 * nl_steinhardt -> nl_solid_bonds(threshold, count) -> nl_clusters(r_max, count, n_min, ...): a particle with at least n_min solid
 * bonds is solid, and solid particles within r_max of each other share a cluster.  The rule of nl_clusters:
 *   - Members.  member_dev == NULL: every particle.  Otherwise member_dev is int32 [n] on the device and particle i is a member
 *     iff member_dev[i] >= min_member: a 0/1 mask (min_member 1), a type array, or the counts of nl_solid_bonds.
 *   - Edges.  An entry (row i, partner j) of the list of the last build is an edge iff i and j are members and r2 < X: the
 *     filtered list where an exclusion or type table is set, so an excluded pair is no edge.  d, r2 and X are those of
 *     nl_pair_histogram: d = r_i - r_j at the image of nl_lj_forces (lj_image), r2 = (dx dx + dy dy) + dz dz in the position
 *     type T without FMA, X the largest T <= r_max r_max taken in double.  A coincident pair (r2 == 0) is an edge, a NaN r2 is
 *     none.  After a NL_LIST_FULL build only the entries with j > i are used.  The graph is undirected, and periodic images
 *     connect as the list found them (a cluster may span the box).
 *   - Output, all written and never added to.  labels_dev, int32 [n]: the smallest particle index of the member's cluster, -1 for
 *     a non-member -- the canonical label, which makes the answer unique.  sizes_dev, int32 [n] or NULL: the number of members
 *     of the member's cluster, 0 for a non-member.  summary_dev, int64 [4] or NULL: {members, clusters, size of the largest
 *     cluster, its label}, ties to the smallest label; without a member the last two are 0 and -1.
 *   - Lists served: NL_LIST_HALF and NL_LIST_FULL lists of whole single-device builds.  A cluster spans ranks: slab and
 *     distributed builds, local-index ones included, are NL_ERR_STATE.
 *   - Arguments and reach.  r_max > 0 and finite and labels_dev != NULL, else NL_ERR_ARG.  The reach is the untyped
 *     histogram's: r_max <= rc, and with a type table r_max <= min_ab rc_ab; the enqueue variant: the same less the skin.
 *   - Ordering, state and n == 0 (nothing is written): those of nl_pair_histogram, checks in the same order.  The enqueue
 *     variant copies nothing from the host; where it finds a non-zero status word it writes -1 to every label, 0 to every size
 *     and -1 to all four summary words, and the error itself surfaces at the next nl_synchronize.
 *   - Scratch: none where sizes_dev is given or summary_dev is not (labels_dev is the parent array of the union-find, sizes_dev
 *     its counters): such a call can be captured from the first one on.  A call with summary_dev and without sizes_dev keeps its
 *     counters in int32 [n_max] of the handle, allocated by the first such call (NL_ERR_STATE inside a capture: make one call
 *     before) and anew by the first after an nl_initialize with another n_max.
 *   - Exact and reproducible.  A lock-free union-find that hooks the larger root under the smaller: the root of a finished
 *     component is its smallest index whatever the schedule, and all counts are integer adds.  Two calls, two builds of one
 *     input (the order of a row's partners differs from build to build) and a half and a full build write the same bytes.
 *   - Five kernels of 256 threads in the stream's order: parent[i] = i; one wave per row over the histogram's walk, unite(i, j)
 *     per edge; labels and counts; sizes and summary; the summary's last two words.  No kernel waits for another workgroup.
 * The rule of nl_solid_bonds, in T, every operation + - x or a correctly rounded sqrt, no FMA:
 *   - The q_lm are those the last nl_steinhardt or nl_steinhardt_enqueue call on this handle left (nl_steinhardt_get_qlm), l
 *     that call's; the neighbour range r_max is the setting's.  Calling nl_steinhardt on this list and these positions first is
 *     the caller's job: the call cannot tell q_lm of other positions from these.
 *   - The neighbours of i are Steinhardt's: the entries j of row i with 0 < r2 < X.
 *   - D_ij = (re_i0 re_j0 + im_i0 im_j0) + 2 S,  S = sum over m = 1 .. l in ascending order of (re_im re_jm + im_im im_jm), 2 S
 *     taken as S + S;  s_i = D_ii.  The bond is solid iff D_ij > (T)threshold sqrt(s_i s_j); no division is taken.
 *   - A NaN on either side makes the bond not solid: a particle with N_b = 0 has NaN q_lm and counts 0, and it is nobody's
 *     neighbour anyway.
 *   - count_dev, int32 [n]: the number of solid bonds of row i, written.
 *   - Lists, reach, ordering, state and n == 0: those of nl_steinhardt (NL_LIST_FULL lists of whole builds; NL_ERR_STATE
 *     without a setting) and, behind them, NL_ERR_STATE where nl_steinhardt_get_qlm would return it.  -1 < threshold < 1, else
 *     NL_ERR_ARG.  The enqueue variant on a failed list writes -1 to every count.  No call allocates.
 *   - One wave per row, one gathered read of 2 (l + 1) values per neighbour, one sum across the wave per row; no atomic, so two
 *     calls write the same bytes.
 * Edges along solid bonds only (freud's SolidLiquid) are another rule and not offered.
 * Tested contract (tests/test_clusters.py): labels, sizes and summary equal, element for element, to an
 * O(N^2) float64 pair search followed by scipy's connected_components wherever no pair lies within 2^-17 (fp32; 2^-46 fp64;
 * relative, r^2) of X; the counts equal to a float64 evaluation wherever no bond lies within SOLID_C u S of the threshold, and
 * bracketed by the sure and the banded bonds elsewhere. */
int nl_clusters(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, const int32_t* member_dev, int32_t min_member,
                int32_t* labels_dev, int32_t* sizes_dev, int64_t* summary_dev, void* stream);
int nl_clusters_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double r_max, const int32_t* member_dev,
                        int32_t min_member, int32_t* labels_dev, int32_t* sizes_dev, int64_t* summary_dev, void* stream);
int nl_solid_bonds(nl_handle_t h, const void* q_dev, int32_t q_stride, double threshold, int32_t* count_dev, void* stream);
int nl_solid_bonds_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, double threshold, int32_t* count_dev, void* stream);

/* Common neighbour analysis from the list: the crystal structure every particle sits in -- fcc, hcp, bcc, icosahedral or none of
 * them -- from the Honeycutt-Andersen / Faken-Jonsson signatures of its bonds, with one fixed cut-off (NL_CNA_FIXED) or with
 * Stukowski's per-particle cut-off (NL_CNA_ADAPTIVE, the rule as OVITO applies it).  All common neighbours of i and k are
 * neighbours of i, so a centre is analysed from its own row and the positions alone.  The rule, every operation in the position
 * type T, + - x / or a correctly rounded sqrt, one rounding each, no FMA:
 *   - Candidates.  The candidates of a centre i are the entries j of row i of the list of the last build with 0 < r2 < X: the
 *     filtered list where an exclusion or type table is set.  d, r2 and X are Steinhardt's: d = r_i - r_j at the image of
 *     nl_lj_forces (lj_image), r2 = (dx dx + dy dy) + dz dz, X the largest T <= r_max r_max taken in double.  N_b is their
 *     number.  A centre with N_b > NL_CNA_MAX_NEAR has no analysis: type NL_CNA_OTHER, bit 0 of its flags set, and it is counted
 *     in word 5 of the summary (and in word 0, as every OTHER).
 *   - Ranking.  The candidates are ranked by (r2, j) ascending; j is unique in a row (a box has at least 3 cells on an axis).
 *   - The set and its bond threshold Y.
 *       FIXED:     the set is all candidates, Y = X.
 *       ADAPTIVE:  K = 1.2071067811865475 (the double nearest (1 + sqrt 2) / 2) rounded to T.
 *                  the 12-set: the ranks 0 .. 11;  S = sum of sqrt(r2) in rank order, starting from the term of rank 0, one
 *                  rounding per add;  c = (S / (T)12) K;  Y = c c.
 *                  the 14-set: the ranks 0 .. 13;  S = the terms sqrt(r2 / (T)0.75) of the ranks 0 .. 7, then sqrt(r2) of the ranks
 *                  8 .. 13, in rank order;  c = (S / (T)14) K;  Y = c c.
 *   - Bonds.  Two members k and m of the set are bonded iff e = d_k - d_m, taken per component, has (ex ex + ey ey) + ez ez < Y
 *     (two coincident members are bonded).  These are distances between the images the list found: with at least 3 cells of
 *     edge >= rc on every periodic axis and r_max <= rc, both members lie within r_max of the centre, so every other image of
 *     the pair (k, m) is at least L - 2 r_max >= rc apart: beyond a fixed threshold (sqrt Y <= rc), and beyond an adaptive one
 *     (sqrt Y <= K r_max) wherever r_max <= rc / K.  The rule is the one stated either way: the images the list found.
 *   - The signature of the bond (i, k), k a member: C = the members bonded to k (the common neighbours); ncn = |C|; nb = the
 *     number of bonded unordered pairs inside C; lc = the largest number of bonds in one connected component of the graph
 *     (C, those bonds) -- OVITO's "maximum chain length".  Counted: n421 = the members with (ncn, nb, lc) = (4, 2, 1), n422 with
 *     (4, 2, 2), n444 with (4, 4, 4), n555 with (5, 5, 5), n666 with (6, 6, 6).
 *   - Type of a set.  12-signature types: FCC iff n421 == 12, else HCP iff n421 == 6 and n422 == 6, else ICO iff n555 == 12.
 *     14-signature type: BCC iff n444 == 6 and n666 == 8.
 *       FIXED:     the set is analysed whatever its size; the type is the 12-signature type where N_b == 12, the 14-signature
 *                  type where N_b == 14, else OTHER.
 *       ADAPTIVE:  N_b < 12: nothing is analysed, OTHER.  Else the 12-set is analysed; where it gives none of FCC, HCP, ICO and
 *                  N_b >= 14 the 14-set is analysed and gives BCC or OTHER; otherwise OTHER.
 *   - Outputs, all written and never added to.  type_dev, int32 [n].  counts_dev, int32 [n][8] or NULL: {N_b (exact, also where
 *     it exceeds 64), size of the last set analysed (0 if none), n421, n422, n444, n555, n666 of that set (0 if none), flags}.
 *     summary_dev, int64 [6] or NULL: {OTHER, FCC, HCP, BCC, ICO, overflowed centres}, zeroed by the call and added to with
 *     integer atomics: exact, the histogram of type_dev.
 *   - Lists served, reach, ordering, state and capture: those of nl_steinhardt and nl_steinhardt_enqueue, checks in the same
 *     order.  NL_LIST_FULL lists of whole single-device builds; a NL_LIST_HALF build, a slab build (local-index ones included)
 *     and a distributed build are NL_ERR_STATE.  r_max > 0 and finite, mode NL_CNA_FIXED or NL_CNA_ADAPTIVE, type_dev != NULL,
 *     else NL_ERR_ARG; r_max <= rc, and with a type table r_max <= rc_ab for every pair of types with rc_ab > 0 (the enqueue
 *     variant: the same less the skin), else NL_ERR_ARG.  n == 0: nothing is written.  The enqueue variant copies nothing from
 *     the host; where it finds a non-zero status word it writes -1 to every type, every counts word and every summary word, and
 *     the error itself surfaces at the next nl_synchronize.  The list is not touched: the next nl_update_list does not build
 *     because of a call.
 *   - No scratch on the handle and no setting: the first call can be captured.  No floating-point atomic: two calls on the same
 *     list and positions write the same bytes.
 *   - One kernel of 256 threads, one wave per centre (k_cna, nl_cna.inc), behind a one-block kernel that zeroes the summary.
 * For the adaptive mode any r_max that holds at least 14 candidates of every particle of interest and at most 64 of any serves;
 * the conventional fixed cut-offs are md_neighbor_list_amd.cna.default_r_max.  Diamond-structure CNA, per-bond signatures and
 * more than 64 candidates are not offered.
 * Tested contract (tests/test_cna.py): type and all eight counts words equal to an O(N^2) float64
 * evaluation of this rule at every particle none of whose decisions lies within 2^-17 (fp32; 2^-46 fp64; relative, r^2) of its
 * threshold; the summary equal to the histogram of the types at all particles. */
enum { NL_CNA_OTHER = 0, NL_CNA_FCC = 1, NL_CNA_HCP = 2, NL_CNA_BCC = 3, NL_CNA_ICO = 4 }; /* OVITO's numbering */
enum { NL_CNA_FIXED = 0, NL_CNA_ADAPTIVE = 1 };
#define NL_CNA_MAX_NEAR 64
int nl_cna(nl_handle_t h, const void* q_dev, int32_t q_stride, int mode, double r_max, int32_t* type_dev, int32_t* counts_dev,
           int64_t* summary_dev, void* stream);
int nl_cna_enqueue(nl_handle_t h, const void* q_dev, int32_t q_stride, int mode, double r_max, int32_t* type_dev,
                   int32_t* counts_dev, int64_t* summary_dev, void* stream);

/* ------------------------------------------------------------------------------------------- introspection */

int nl_get_mesh(nl_handle_t h, int32_t mesh[3], int64_t* ncell);
/* Cell-sorted state of the last build, for tests of the hash/sort stage (a3-a5 of SURVEY.md section 8):
 * cell_start[ncell_local + 1]; sorted positions {x,y,z,id} (16 B for F32, 32 B {double x,y,z; int32 id,row}
 * for F64); sorted_row[n] = input index of each sorted slot.  After a fine-row build (nl_get_build_info, info[6] != 0)
 * the cell's particles are additionally ordered by the quarter of the cell they lie in along z and the table has
 * 4 * ncell_local + 1 entries: entry (cell * 4 + quarter) = first slot of that quarter; every fourth entry is the
 * cell_start of the plain build. */
int nl_get_sorted(nl_handle_t h, const int32_t** cell_start_dev, const void** sorted_pos_dev,
                  const int32_t** sorted_row_dev, int64_t* ncell_local);
/* Diagnostic cycle accumulators of the kernels (filled only when NL_DEBUG_FLAGS & 4 is set in the environment). */
int nl_debug_read(nl_handle_t h, uint64_t* out, int32_t n, int reset);
int nl_debug_occupancy(int32_t out[8]); /* LDS per CU/block (KiB), occupancy API answers, LDS bytes, registers */
/* How the last build was organised: info[0] = 1 when the COUNT sweep kept hit masks and the list was expanded from
 * them (0: two distance sweeps), info[1] = configured sweep variant, info[2] = LDS batch capacity (particles),
 * info[3] = compute units of the device, info[4] = width of the list offsets the build used (32 / 64), info[5] = mask rows per particle (1; up to 7 in a
 * dense build: one per LDS batch of the stencil stream), info[6] = 0, or 1 + c when the build took the fine-row search
 * (nl_rows.hpp; c = its LDS configuration 0..2) -- the table nl_get_sorted returns is then the fine-row table,
 * info[7] = 1 when the build used the small instances of the COUNT sweep and the expansion (sparse boxes: 2 waves /
 * 1 wave per cell, half the LDS buffer), else 0; bits 8..15 of info[7] = C when the build took the id-class search
 * (k_sweep_class_f32: C = 2 or 4 classes of ids; NL_IDCLASS), else 0; bits 16..17 of info[7] = the binning the build
 * took: 0 = two passes over rows of x-cells, 1 = one pass into row buckets, 2 = atomic ranks into the cell histogram
 * (NL_BINNING=1, and every mesh of more than 12288 rows of x-cells or more than 4096 cells a row; such a build has no
 * fine rows and no id classes); bit 18 of info[7] = 1 when the id-class search ran with the reach cull (partners no
 * particle of the cell can reach leave the staged stream before the search; NL_CULL=0 turns it off).  Asserted on both sides of those limits, lists against the oracle: tests/test_mesh_limits.py. */
int nl_get_build_info(nl_handle_t h, int32_t info[8]);
/* How the builds of this handle ran: stats[0] = builds run again because a row of x-cells overflowed its bucket in the
 * one-pass binning, stats[1] = builds run again because cells whose stencil exceeds the LDS buffer were there while the
 * build had left out the kernels for them, stats[2] = bucket size of the last build's one-pass binning (0: the
 * two-pass binning), stats[3] = 1 when the last build launched those kernels. */
int nl_get_build_stats(nl_handle_t h, int64_t stats[4]);
int nl_last_error(nl_handle_t h);     /* status of the last failed call on this handle */
int nl_last_hip_error(nl_handle_t h); /* raw hipError_t behind the last NL_ERR_HIP */

/* Per-kernel device time of one build, measured with HIP events on the stream the kernels were launched on.
 * Runs `reps` builds of the given positions and returns average milliseconds per build for each stage
 * (NL_STAGE_*) in ms[NL_NUM_STAGES]; ms[NL_STAGE_TOTAL] is first-launch to last-kernel-end. */
enum {
  NL_STAGE_HASH = 0,     /* cell hash + per-cell rank                       */
  NL_STAGE_CELL_SCAN = 1,/* exclusive scan of the cell histogram            */
  NL_STAGE_REORDER = 2,  /* physical reorder of positions into cell order   */
  NL_STAGE_COUNT = 3,    /* pair search, counting pass                      */
  NL_STAGE_ROW_SCAN = 4, /* exclusive scan of the counts -> key_pointer     */
  NL_STAGE_FILL = 5,     /* pair search, list-filling pass                  */
  NL_STAGE_TOTAL = 6,
  NL_NUM_STAGES = 7
};
int nl_profile_stages(nl_handle_t h, const void* q_dev, int32_t q_stride, int32_t n, int32_t reps,
                      double ms[NL_NUM_STAGES]);
/* Same, re-running the last successful build (single-device or slab) with the arguments it was given; the
 * position / id buffers of that build must still be alive.  Not a passive timer: the build is planned again as one whole,
 * ungated build (a begin / finish pair runs as one call; a build that was run again, or an update's, keeps the two-pass
 * binning and every launch it ran with), run `reps` times into the handle's own buffers from the positions the buffer
 * holds now, and adopted -- the list, the plan and nl_get_build_info / nl_get_build_stats afterwards are that build's,
 * and like any build other than an update's it makes the next nl_update_list build (rule (a) above). */
int nl_profile_last_build(nl_handle_t h, int32_t reps, double ms[NL_NUM_STAGES]);

/* --------------------------------------------------------------------------------- buffers (cuda_ptr shim) */

/* Back the reference's cuda_ptr<T> (cuda_ptr.cuh:11-112): a device buffer paired with a pinned host buffer. */
int nl_buf_alloc(void** dev, void** host, size_t bytes);          /* allocate(), cuda_ptr.cuh:40-45; either
                                                                     pointer may be NULL (that half is skipped) */
int nl_buf_free(void* dev, void* host);                           /* deallocate(), cuda_ptr.cuh:107-111    */
int nl_buf_h2d(void* dev, const void* host, size_t bytes);        /* host2dev(), cuda_ptr.cuh:47-53        */
int nl_buf_d2h(void* host, const void* dev, size_t bytes);        /* dev2host(), cuda_ptr.cuh:62-69        */
int nl_buf_fill32(void* dev, uint32_t pattern, size_t count);     /* set_val() device half, cuda_ptr.cuh:79-89 */
int nl_buf_fill64(void* dev, uint64_t pattern, size_t count);
int nl_device_synchronize(void);                                  /* make_list.cu:128                      */
int nl_device_count(int* count);

#ifdef __cplusplus
}
#endif
#endif /* NL_HIP_H */
