"""Python mirror of the reference's builder classes, over the C ABI of libnl_hip.so.

``NeighListGPU`` keeps the call surface of the reference's ``NeighListGPU<Vec,Dtype>`` (neighlist_gpu.hpp:43-488:
ctor, Initialize, MakeNeighList, neigh_list, number_of_partners, number_of_pairs) and adds the accessors of the
scalar CPU class ``NeighList<Vec>`` (neighlist_cpu.hpp:437-463: key_pointer, sorted_list, half counts), because the
CPU class's half CSR is the native output of the HIP path and the contract it is checked against.

torch is plumbing only here: device memory for positions/results and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import NLError, check  # noqa: F401


class _DevView:
    """A borrowed device buffer exposed through __cuda_array_interface__ (zero copy into torch)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {
            "shape": tuple(int(s) for s in shape),
            "typestr": typestr,
            "data": (int(ptr), False),
            "version": 2,
            "strides": None,
        }
        self._owner = owner  # keeps the handle alive


def _as_tensor(ptr, shape, typestr, owner, device):
    n = 1
    for s in shape:
        n *= int(s)
    if n == 0 or not ptr:
        dt = {"|i1": torch.int8, "<i4": torch.int32, "<i8": torch.int64, "<f4": torch.float32, "<f8": torch.float64}[typestr]
        return torch.empty(tuple(int(s) for s in shape), dtype=dt, device=device)
    return torch.as_tensor(_DevView(ptr, shape, typestr, owner), device=device)


class NeighListGPU:
    """Verlet neighbour-list builder on one MI355X.

    Parameters follow neighlist_gpu.hpp:236-255: ``search_length`` (cut-off rc) and the box edges.  ``dtype``
    plays the role of the reference's compile-time ``Dtype``/``Vec`` choice (make_list.cu:6-12).  ``minimum_image``:
    False (the reference's open box), True (every axis periodic), or the periodic axes as in ``set_periodic(axes=)``.
    ``tilt``: (xy, xz, yz) of a triclinic box (``set_box``); a tilt needs both of its axes periodic.
    """

    def __init__(self, search_length, Lx, Ly, Lz, dtype=torch.float32, device=None, full_list=False,
                 minimum_image=False, tilt=None):
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("dtype must be torch.float32 or torch.float64")
        self._lib = _lib.load()  # raises when the HIP extension is missing
        if not torch.cuda.is_available():
            raise RuntimeError("NeighListGPU needs a HIP device; there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.dtype = dtype
        self.search_length = float(search_length)
        self._h = C.c_void_p()
        check(
            self._lib.nl_create(C.byref(self._h), _lib.NL_F32 if dtype == torch.float32 else _lib.NL_F64,
                                float(search_length), float(Lx), float(Ly), float(Lz), self.device.index or 0),
            "nl_create",
        )
        self._read_mesh()
        self._n = 0
        self._n_rows = 0
        self.full_list = False
        self.minimum_image = False
        self.periodic_axes = (False, False, False)
        if full_list:
            self.set_full_list(True)
        if minimum_image:
            self.set_periodic(axes=minimum_image)
        if tilt is not None and any(float(t) != 0.0 for t in tilt):
            self.set_box(Lx, Ly, Lz, *(float(t) for t in tilt))
        self._q = None  # keeps the positions of an asynchronous build alive
        self._charges = None  # set_charges
        self.skin = 0.0

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.nl_destroy(h)
            except Exception:  # pragma: no cover
                pass

    # ------------------------------------------------------------------ reference surface
    def Initialize(self, particle_number):
        """neighlist_gpu.hpp:268-287 / neighlist_cpu.hpp:408-415."""
        check(self._lib.nl_initialize(self._h, int(particle_number)), "nl_initialize")

    def set_capacity(self, max_pairs):
        check(self._lib.nl_set_capacity(self._h, int(max_pairs)), "nl_set_capacity")

    def set_offset_width(self, bits=0):
        """Width of the list offsets (nl_set_offset_width): 0 = 64-bit as soon as the list capacity exceeds INT32_MAX
        entries, 32 / 64 = forced.  The reference's int32 offsets wrap beyond 2^31 pairs (neighlist_cpu.hpp:15,29)."""
        check(self._lib.nl_set_offset_width(self._h, int(bits)), "nl_set_offset_width")

    def set_graph(self, on: bool = True):
        """Replay asynchronous builds from a captured hipGraph (nl_set_graph): saves launch overhead on small systems."""
        check(self._lib.nl_set_graph(self._h, 1 if on else 0), "nl_set_graph")

    def set_local_ids(self, on: bool = True):
        """Local-index slab lists (nl_set_local_ids): slab builds then take ``gid=None`` only, their ids are rows of the
        caller's buffer (owned rows first, ghosts behind them), and lj_forces, lj_virial and pair_histogram read them, one
        rank's share each.  Synchronous; a changed value drops the list.  Off by default."""
        check(self._lib.nl_set_local_ids(self._h, 1 if on else 0), "nl_set_local_ids")

    @property
    def local_ids(self):
        """Whether slab builds are local-index lists that the consumers accept (nl_get_local_ids)."""
        on = C.c_int()
        check(self._lib.nl_get_local_ids(self._h, C.byref(on)), "nl_get_local_ids")
        return bool(on.value)

    def set_periodic(self, minimum_image=True, axes=None):
        """Minimum-image distances across the periodic faces (nl_set_periodic_axes).  The reference, and the default
        here, wrap the cell stencil but measure distances in an open box.  ``axes`` picks the periodic axes: a 3-tuple
        of bools or a string drawn from "xyz" (``axes="xy"``: a film, open in z); ``None`` = all three when
        ``minimum_image`` is true, none otherwise.  ``minimum_image`` is True only for a fully periodic box."""
        mask = axes_mask(bool(minimum_image) if axes is None else axes)
        check(self._lib.nl_set_periodic_axes(self._h, mask), "nl_set_periodic_axes")
        self.periodic_axes = tuple(bool(mask >> d & 1) for d in range(3))
        self.minimum_image = mask == 7

    def set_box(self, Lx, Ly, Lz, xy=0.0, xz=0.0, yz=0.0):
        """A new box for the next builds (nl_set_box): edge vectors a = (Lx, 0, 0), b = (xy, Ly, 0), c = (xz, yz, Lz)
        (LAMMPS convention, origin 0).  Synchronous; a changed box drops the list and the next update builds.  Exclusion
        and type tables, the skin and the periodic axes are kept; ``mesh_size`` follows the new box."""
        check(self._lib.nl_set_box(self._h, float(Lx), float(Ly), float(Lz), float(xy), float(xz), float(yz)), "nl_set_box")
        self._read_mesh()

    @property
    def box(self):
        """(Lx, Ly, Lz, xy, xz, yz) of the next build (nl_get_box)."""
        b = (C.c_double * 6)()
        check(self._lib.nl_get_box(self._h, C.byref(b)), "nl_get_box")
        return tuple(float(v) for v in b)

    def _read_mesh(self):
        mesh = (C.c_int32 * 3)()
        ncell = C.c_int64()
        check(self._lib.nl_get_mesh(self._h, C.byref(mesh), C.byref(ncell)))
        self.mesh_size = tuple(mesh)
        self.number_of_mesh = int(ncell.value)

    def periodic_mask(self):
        """The axis mask the next build uses (nl_get_periodic_axes): bit 0 = x, bit 1 = y, bit 2 = z."""
        m = C.c_int()
        check(self._lib.nl_get_periodic_axes(self._h, C.byref(m)), "nl_get_periodic_axes")
        return int(m.value)

    def set_full_list(self, full=True):
        """Builds produce the FULL list (every pair in both rows: the reference GPU kernels' contract,
        kernel_impl.cuh:24-33) instead of the scalar CPU class's half list; ``neigh_list()`` is then one coalesced
        conversion pass away.  The half-list accessors raise after a full build and vice versa."""
        check(self._lib.nl_set_list_kind(self._h, 1 if full else 0), "nl_set_list_kind")
        self.full_list = bool(full)

    def _check_q(self, q, n):
        if not isinstance(q, torch.Tensor) or q.device.type != "cuda":
            raise TypeError("q must be a torch tensor on the HIP device")
        if q.dtype != self.dtype or q.dim() != 2 or q.shape[1] not in (3, 4) or not q.is_contiguous():
            raise TypeError(f"q must be a contiguous (N, 3|4) tensor of {self.dtype}")
        n = q.shape[0] if n is None else int(n)
        if n > q.shape[0]:
            raise ValueError("particle_number exceeds the buffer")
        return n

    def MakeNeighList(self, q, particle_number=None, sync=True, tblock_size=128, smem_hei=7):
        """neighlist_gpu.hpp:289-466.  ``tblock_size``/``smem_hei`` select among the reference's CUDA variants
        and are accepted for source compatibility only."""
        n = self._check_q(q, particle_number)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._q = q
        self._n = self._n_rows = n
        check(self._lib.nl_make_list(self._h, q.data_ptr(), q.shape[1], n, stream, 1 if sync else 0), "nl_make_list")

    # ------------------------------------------------------------------ Verlet-skin updates
    def set_skin(self, skin):
        """Skin of the Verlet list (nl_set_skin): the handle's cut-off is the physical cut-off + skin, and update() keeps
        the list until some particle has moved more than skin / 2 since its build."""
        check(self._lib.nl_set_skin(self._h, float(skin)), "nl_set_skin")
        self.skin = float(skin)

    def update(self, q, particle_number=None, sync=False):
        """Rebuilds the list only where it no longer holds (nl_update_list): decided on the device, in stream order, with
        no host wait -- so that an MD step can be enqueued ahead or captured into a graph.  ``sync=True`` waits and grows
        the list like ``MakeNeighList(sync=True)``."""
        n = self._check_q(q, particle_number)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._q = q
        self._n = self._n_rows = n
        check(self._lib.nl_update_list(self._h, q.data_ptr(), q.shape[1], n, stream, 1 if sync else 0), "nl_update_list")

    def update_stats(self):
        """(updates, builds they performed) of this handle (nl_get_update_stats; waits for the device)."""
        st = (C.c_int64 * 2)()
        check(self._lib.nl_get_update_stats(self._h, C.byref(st)), "nl_get_update_stats")
        return int(st[0]), int(st[1])

    # ------------------------------------------------------------------ excluded pairs
    def _int32_input(self, a, name, shape, dims, word):
        """A caller's int32/int64 tensor or array as a contiguous int32 device tensor.  dims: its shape, None for any extent;
        name, shape and word fill the messages.  int64 values outside the int32 range are refused: a cast would wrap them."""
        if isinstance(a, torch.Tensor):
            t = a
        else:
            import numpy as np

            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        if t.dtype not in (torch.int32, torch.int64) or t.dim() != len(dims) or any(d is not None and e != d for e, d in zip(t.shape, dims)):
            raise TypeError(f"{name} must be an {shape} int32 or int64 tensor or array")
        if t.dtype == torch.int64 and t.numel() and (int(t.min()) < -2**31 or int(t.max()) >= 2**31):
            raise ValueError(f"{name} hold {word} outside the int32 range")
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def _exclusion_pairs(self, pairs):
        return self._int32_input(pairs, "pairs", "(E, 2)", (None, 2), "an index")

    def set_exclusions(self, pairs, particle_number):
        """Leaves the pairs of ``pairs`` out of every later build (nl_set_exclusions): an ``(E, 2)`` int32/int64 tensor or
        array of input-order particle indices (duplicates and both orders allowed) for builds of ``particle_number``
        particles.  Bonded partners of a molecular model; capacity is still counted before exclusion."""
        t = self._exclusion_pairs(pairs)
        check(self._lib.nl_set_exclusions(self._h, t.data_ptr() if t.shape[0] else None, int(t.shape[0]), int(particle_number)),
              "nl_set_exclusions")

    def set_exclusions_global(self, pairs, n_ids):
        """Leaves the pairs of ``pairs`` out of every later build, keyed by the ids the list stores
        (nl_set_exclusions_global): an ``(E, 2)`` int32/int64 tensor or array of ids in ``[0, n_ids)`` -- the global
        tags of a decomposed run, the same table on every rank.  Applies to slab builds (any id form), the begin /
        finish pair, distributed builds and whole builds; replaces a table set by ``set_exclusions`` and is never
        relabelled by ``resort()``.  The handle holds 4 bytes per global id."""
        t = self._exclusion_pairs(pairs)
        check(self._lib.nl_set_exclusions_global(self._h, t.data_ptr() if t.shape[0] else None, int(t.shape[0]), int(n_ids)),
              "nl_set_exclusions_global")

    def clear_exclusions(self):
        """Drops the exclusion table: later builds list every pair again."""
        check(self._lib.nl_set_exclusions(self._h, None, 0, 0), "nl_set_exclusions")

    def exclusions(self):
        """(offsets[n + 1], ids) of the exclusion table (nl_get_exclusions): symmetric, per-row ascending, without
        duplicates; views valid until the table is set, cleared or relabelled by resort()."""
        off, ids, n, nu = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int64()
        check(self._lib.nl_get_exclusions(self._h, C.byref(off), C.byref(ids), C.byref(n), C.byref(nu)), "nl_get_exclusions")
        return (_as_tensor(off.value, (n.value + 1,), "<i4", self, self.device),
                _as_tensor(ids.value, (2 * nu.value,), "<i4", self, self.device))

    # ------------------------------------------------------------------ per-type cut-offs
    def set_type_cutoffs(self, types, rc_matrix):
        """Cut-offs per pair of particle types (nl_set_type_cutoffs): ``types`` an ``(n,)`` int32/int64 tensor or array in
        input order, ``rc_matrix`` an ``(ntypes, ntypes)`` symmetric matrix with entries in [0, search_length] (skin
        included).  Every later build keeps an entry only within the cut-off of its two types."""
        import numpy as np

        rc = np.ascontiguousarray(np.asarray(rc_matrix, dtype=np.float64))
        if rc.ndim != 2 or rc.shape[0] != rc.shape[1]:
            raise TypeError("rc_matrix must be a square (ntypes, ntypes) matrix")
        t = self._int32_input(types, "types", "(n,)", (None,), "a value")
        n = int(t.shape[0])
        ptr = t.data_ptr() if n else None
        if n == 0:  # (an empty table still needs a non-NULL pointer: NULL clears)
            t = torch.zeros(1, dtype=torch.int32, device=self.device)
            ptr = t.data_ptr()
        check(self._lib.nl_set_type_cutoffs(self._h, ptr, n, int(rc.shape[0]), rc.ctypes.data_as(C.POINTER(C.c_double))),
              "nl_set_type_cutoffs")

    def clear_type_cutoffs(self):
        """Drops the type table: later builds use the one cut-off again."""
        check(self._lib.nl_set_type_cutoffs(self._h, None, 0, 0, None), "nl_set_type_cutoffs")

    def types(self):
        """The handle's copy of the types (nl_get_types), relabelled by resort(); a view, valid until the table is set
        or cleared."""
        ptr, n, _ = self._get_types()
        return _as_tensor(ptr, (n,), "<i4", self, self.device)

    def _get_types(self):
        """(pointer, n, ntypes) of the handle's type table (nl_get_types; NL_ERR_STATE without one)."""
        ptr, n, nt = C.c_void_p(), C.c_int32(), C.c_int32()
        check(self._lib.nl_get_types(self._h, C.byref(ptr), C.byref(n), C.byref(nt)), "nl_get_types")
        return ptr.value, int(n.value), int(nt.value)

    def set_lj_type_params(self, epsilon, sigma, rc_force):
        """Lennard-Jones parameters per pair of types for lj_forces_typed (nl_set_lj_type_params): three symmetric
        ``(ntypes, ntypes)`` matrices, rc_force within the type table's cut-offs."""
        import numpy as np

        mats = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in (epsilon, sigma, rc_force)]
        nt = mats[0].shape[0] if mats[0].ndim == 2 else -1
        if any(m.shape != (nt, nt) for m in mats):
            raise TypeError("epsilon, sigma and rc_force must be (ntypes, ntypes) matrices")
        ptrs = [m.ctypes.data_as(C.POINTER(C.c_double)) for m in mats]
        check(self._lib.nl_set_lj_type_params(self._h, int(nt), *ptrs), "nl_set_lj_type_params")

    def lj_forces_typed(self, q, wait=True, out=None):
        """lj_forces with the parameters of set_lj_type_params, per pair of types (nl_lj_forces_typed); ``wait=False``:
        nl_lj_forces_typed_enqueue (rc_force within cut-off - skin).  Returns ``(n, 4) = {fx, fy, fz, pe_i}``."""
        return self._consume("nl_lj_forces_typed", q, (), wait, out, totals=False)

    # ------------------------------------------------------------------ pair images
    def set_pair_images(self, on=True):
        """Builds also report the periodic image of every entry (nl_set_pair_images): the integer triple s with
        q_j + s_a a + s_b b + s_c c - q_i the displacement at which the search found the pair -- the ``S`` of ASE's
        ``neighbour_list("ijS")``, the ``shifts`` of an ``edge_index`` consumer.  Synchronous; a changed value drops the list.
        While on, update() takes its skin check without the minimum-image fold: re-wrapping a particle into the box rebuilds."""
        check(self._lib.nl_set_pair_images(self._h, 1 if on else 0), "nl_set_pair_images")

    def pair_images(self):
        """int8 ``[P, 3]`` images of the entries of the last build (nl_get_pair_images), entry k at the index of
        ``sorted_list()[k]`` / ``full_csr()[1][k]``: a view of the ``[P, 4]`` buffer, valid until the next build."""
        ptr, ne = C.c_void_p(), C.c_int64()
        check(self._lib.nl_get_pair_images(self._h, C.byref(ptr), C.byref(ne)), "nl_get_pair_images")
        return _as_tensor(ptr.value, (ne.value, 4), "|i1", self, self.device)[:, :3]

    def pair_vectors(self, q, out=None, wait=True):
        """``[P, 4] = {dx, dy, dz, r2}`` of every entry of the last build at its image, r_j - r_i (nl_pair_vectors), from
        ``q``: the build's positions or positions moved within the skin.  ``wait=False`` (nl_pair_vectors_enqueue): no
        wait for the build, stream-ordered behind the last update(); ``out`` is then required and must hold the list's
        capacity, and a list whose build failed gives NaN.  ``out``: a contiguous ``[>= P, 4]`` tensor to write into."""
        n = self._check_q(q, None)
        if n != self._n:
            raise ValueError("q must hold the particles the list was built from")
        entries = None
        if wait:  # the count the library reports with the images (NL_ERR_STATE with the flag off or without a build)
            ne = C.c_int64()
            check(self._lib.nl_get_pair_images(self._h, None, C.byref(ne)), "nl_get_pair_images")
            entries = int(ne.value)
        if out is None:
            if not wait:
                raise ValueError("pair_vectors(wait=False) needs out= with room for the list's capacity")
            out = torch.empty((entries, 4), dtype=self.dtype, device=self.device)
        if out.dim() != 2 or out.shape[1] != 4 or out.dtype != self.dtype or not out.is_contiguous() or out.device.type != "cuda":
            raise TypeError("out must be a contiguous (P, 4) device tensor of the list's dtype")
        if wait and out.shape[0] < entries:
            raise ValueError("out is shorter than the list")
        target = out
        if out.numel() == 0:  # (torch gives an empty tensor no address: the call still runs, and reports its errors)
            if not wait:
                raise ValueError("pair_vectors(wait=False) needs out= with room for the list's capacity")
            target = torch.empty((1, 4), dtype=self.dtype, device=self.device)  # (an empty list: nothing is written)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        fn = self._lib.nl_pair_vectors if wait else self._lib.nl_pair_vectors_enqueue
        check(fn(self._h, q.data_ptr(), q.shape[1], target.data_ptr(), stream), "nl_pair_vectors" if wait else "nl_pair_vectors_enqueue")
        return out

    def list_entries(self):
        """Entries of the last list as the library counts them (npairs of nl_get_half_csr, nentries of nl_get_full_csr;
        waits for the build).  Not 2 x number_of_pairs: the two rows of a full list decide a pair on their own and may
        differ within one ulp of the cut-off across a periodic face, so a full list can hold an odd number of entries."""
        return (self._full(0) if self.full_list else self._half(0))[3]

    def edge_index(self):
        """``[2, P]`` int64 (row, partner) of every entry of the last build, in the order of pair_images() and
        pair_vectors(): the ``edge_index`` of a PyTorch consumer.  Plumbing over the CSR; a copy."""
        if self.full_list:
            _kp, lst, cnt = self.full_csr(64)
        else:
            lst, cnt = self.sorted_list(), self.half_number_of_partners()
        rows = torch.repeat_interleave(torch.arange(self._n_rows, dtype=torch.int64, device=self.device), cnt.to(torch.int64),
                                       output_size=int(lst.shape[0]))
        return torch.stack([rows, lst.to(torch.int64)])

    GID_IN_W = "w"  # MakeNeighListSlab(gid=GID_IN_W): ids are stored in q[:, 3] as integer bit patterns (NL_GID_IN_W)

    def _gid_ptr(self, q, gid, n):
        """What a slab build takes as gid: the tensor's address, NULL for None (identity), 1 for GID_IN_W."""
        if isinstance(gid, str):
            if gid != self.GID_IN_W or q.shape[1] != 4:
                raise TypeError("gid='w' needs 4-component positions")
            return 1
        if gid is None:
            return None
        if gid.device.type != "cuda" or gid.dtype != torch.int32 or gid.numel() != n or not gid.is_contiguous():
            raise TypeError("gid must be a contiguous int32 device tensor with one id per particle")
        return gid.data_ptr()

    def MakeNeighListSlab(self, q, gid, n_rows, z_lo, z_hi, sync=True):
        """Domain-decomposed build: rows for the first ``n_rows`` (owned) particles, the rest
        are ghosts of the two neighbouring cell layers; ``gid`` are global ids: an int32 device tensor, None
        (identity) or ``GID_IN_W`` (taken from the w component of the positions)."""
        n = self._check_q(q, None)
        gid_ptr = self._gid_ptr(q, gid, n)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._q = (q, gid)
        self._n, self._n_rows = n, int(n_rows)
        check(
            self._lib.nl_make_list_slab(self._h, q.data_ptr(), q.shape[1], gid_ptr, int(n_rows), n, int(z_lo), int(z_hi),
                                        stream, 1 if sync else 0),
            "nl_make_list_slab",
        )

    def MakeNeighListSlabBegin(self, q, gid, n_rows, n_ghost_lo, z_lo, z_hi):
        """nl_make_list_slab_begin: the part of a slab build that needs only the owned particles q[:n_rows]; the ghost
        rows of q may still be in flight.  Follow with MakeNeighListSlabFinish once the current stream waits for them."""
        n = self._check_q(q, None)
        gid_ptr = self._gid_ptr(q, gid, n)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._q = (q, gid)
        self._n, self._n_rows = n, int(n_rows)
        check(
            self._lib.nl_make_list_slab_begin(self._h, q.data_ptr(), q.shape[1], gid_ptr, int(n_rows), n, int(n_ghost_lo),
                                              int(z_lo), int(z_hi), stream),
            "nl_make_list_slab_begin",
        )

    def MakeNeighListSlabFinish(self, sync=True):
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self._lib.nl_make_list_slab_finish(self._h, stream, 1 if sync else 0), "nl_make_list_slab_finish")

    def synchronize(self):
        check(self._lib.nl_synchronize(self._h), "nl_synchronize")

    def neigh_list(self):
        """neighlist_gpu.hpp:468-474: full list, transposed, ``[k, i]`` = k-th neighbour of i for ``k < count[i]``
        (nl_get_full_transposed); the number of columns is the n of the last build.  Entries ``k >= count[i]`` hold -1
        after a half build, and after a full build when the buffer was just allocated or grown (the first fetch, one
        after ``Initialize`` or ``set_full_list``) -- otherwise whatever an earlier build left there."""
        lst, _, stride, mx = self._full_transposed()
        return _as_tensor(lst, (max(mx, 1), stride), "<i4", self, self.device)

    def _full_transposed(self):
        """(list, counts, stride, longest row) of nl_get_full_transposed."""
        lst, cnt, stride, mx = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int32()
        check(self._lib.nl_get_full_transposed(self._h, C.byref(lst), C.byref(cnt), C.byref(stride), C.byref(mx)),
              "nl_get_full_transposed")
        return lst.value, cnt.value, int(stride.value), int(mx.value)

    def number_of_partners(self):
        """neighlist_gpu.hpp:476-482: full counts."""
        _, cnt, stride, _ = self._full_transposed()
        return _as_tensor(cnt, (stride,), "<i4", self, self.device)

    def number_of_pairs(self):
        """neighlist_gpu.hpp:484-487: the sum of the FULL counts (= 2 x half pairs)."""
        return 2 * self.half_number_of_pairs()

    # ------------------------------------------------------------------ CPU-class surface (half CSR)
    def _half(self, width=32):
        """(key_pointer, sorted_list, counts, npairs) pointers; width = 32 | 64 (key_pointer type) | 0 (no key_pointer)."""
        kp, sl, nop, npairs = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        f = self._lib.nl_get_half_csr if width == 32 else self._lib.nl_get_half_csr64
        check(f(self._h, C.byref(kp) if width else None, C.byref(sl), C.byref(nop), C.byref(npairs)), "nl_get_half_csr")
        return kp.value, sl.value, nop.value, int(npairs.value)

    def _full(self, width=32):
        kp, sl, nop, ne = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        f = self._lib.nl_get_full_csr if width == 32 else self._lib.nl_get_full_csr64
        check(f(self._h, C.byref(kp) if width else None, C.byref(sl), C.byref(nop), C.byref(ne)), "nl_get_full_csr")
        return kp.value, sl.value, nop.value, int(ne.value)

    def full_csr(self, width=32):
        """(key_pointer[N+1], list[2P], counts[N]) of a full-list build, as views valid until the next build."""
        kp, sl, nop, ne = self._full(width)
        return (_as_tensor(kp, (self._n_rows + 1,), "<i4" if width == 32 else "<i8", self, self.device),
                _as_tensor(sl, (ne,), "<i4", self, self.device),
                _as_tensor(nop, (self._n_rows,), "<i4", self, self.device))

    def half_number_of_pairs(self):
        """neighlist_cpu.hpp:437-439."""
        npairs = C.c_int64()
        check(self._lib.nl_number_of_pairs(self._h, C.byref(npairs)), "nl_number_of_pairs")
        return int(npairs.value)

    def key_pointer(self):
        """neighlist_cpu.hpp:449-455 (view, valid until the next build).  int32 like the reference's: raises
        NL_ERR_INDEX_OVERFLOW for a list of more than INT32_MAX entries (use key_pointer64)."""
        kp, _, _, _ = self._half()
        return _as_tensor(kp, (self._n_rows + 1,), "<i4", self, self.device)

    def key_pointer64(self):
        """The same offsets as int64 (nl_get_half_csr64): for lists beyond the reference's int32 limit."""
        kp, _, _, _ = self._half(64)
        return _as_tensor(kp, (self._n_rows + 1,), "<i8", self, self.device)

    def sorted_list(self):
        """neighlist_cpu.hpp:441-447 (view, valid until the next build)."""
        _, sl, _, npairs = self._half(0 if npairs_exceeds_int32(self) else 32)
        return _as_tensor(sl, (npairs,), "<i4", self, self.device)

    def half_number_of_partners(self):
        """neighlist_cpu.hpp:457-463 (view, valid until the next build)."""
        _, _, nop, _ = self._half(0 if npairs_exceeds_int32(self) else 32)
        return _as_tensor(nop, (self._n_rows,), "<i4", self, self.device)

    def list_checksum(self):
        """Order-independent checksum of the last list, computed on the device (nl_list_checksum): the pair-set hash of
        the known answers.  Returns (checksum, entries)."""
        cs, ne = C.c_uint64(), C.c_int64()
        check(self._lib.nl_list_checksum(self._h, C.byref(cs), C.byref(ne)), "nl_list_checksum")
        return int(cs.value), int(ne.value)

    # ------------------------------------------------------------------ a consumer of the list
    def lj_forces(self, q, epsilon=1.0, sigma=1.0, rc_force=None, wait=True, out=None):
        """Truncated Lennard-Jones forces and per-particle energies ``(n, 4) = {fx, fy, fz, pe_i}`` from the list of
        the last build (nl_lj_forces): gather per row after a full-list build, pair-once with atomics after a half
        build.  ``wait=False`` (nl_lj_forces_enqueue): no wait for the build, stream-ordered behind the last update();
        rc_force must then be <= cut-off - skin, and a list whose build failed gives NaN.  ``out``: an (n, 4) tensor
        to write into (graph capture).  After a slab build under set_local_ids: ``(n_rows, 4)``, the owned particles' rows
        of the global result (a ghost partner receives no reaction: its owner evaluates the pair in its own row)."""
        return self._consume("nl_lj_forces", q, (epsilon, sigma, rc_force), wait, out, totals=False)

    def _consume(self, name, q, lj, wait, out, totals, tail=()):
        """The consumers' call: the output (the ``(n_rows, 4)`` rows of the list's dtype, or the 8 float64 ``totals``), the
        stream, the pick of ``name`` or ``name``_enqueue and the call.  lj: (epsilon, sigma, rc_force) for the scalar
        Lennard-Jones forms, () for every other consumer; an argument that is a device pointer (the charges, the velocities)
        is a c_void_p, a stride a c_int32.
        tail: integer arguments between the output and the stream (the ``add`` of coul_excl_forces)."""
        n = self._check_q(q, None)
        if n != self._n:
            raise ValueError("q must hold the particles the list was built from")
        if totals:
            o = torch.empty(8, dtype=torch.float64, device=self.device) if out is None else out
            if o.shape != (8,) or o.dtype != torch.float64 or not o.is_contiguous() or o.device != q.device:
                raise TypeError("out must be a contiguous float64 tensor of 8 on the list's device")
        else:
            rows = self._n_rows  # (a whole build: n)
            o = torch.empty((rows, 4), dtype=self.dtype, device=self.device) if out is None else out
            if o.shape != (rows, 4) or o.dtype != self.dtype or not o.is_contiguous():
                raise TypeError("out must be a contiguous (n_rows, 4) tensor of the list's dtype")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if len(lj) == 3 and lj[2] is None:
            lj = (lj[0], lj[1], self.search_length if wait else self.search_length - self.skin)
        name += "" if wait else "_enqueue"
        extra = (v if isinstance(v, (C.c_void_p, C.c_int32)) else float(v) for v in lj)
        check(getattr(self._lib, name)(self._h, q.data_ptr(), q.shape[1], *extra, o.data_ptr(), *tail, stream), name)
        return o

    def lj_virial(self, q, epsilon=1.0, sigma=1.0, rc_force=None, wait=True, out=None):
        """The totals that belong to lj_forces (nl_lj_virial): a float64 device tensor
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}`` for both dtypes, W_ab = sum over pairs d_a F_b (d = r_i - r_j, F on
        i: repulsion is positive), U the potential energy, n_in the pairs within rc_force; the same for a half and a full
        list, without floating-point atomics and bit for bit reproducible.
        Pressure: ``P = N kT / V + (w[0] + w[1] + w[2]) / (3 V)``.
        ``wait``, ``rc_force`` and ``out`` (a float64 tensor of 8) as for lj_forces; with ``wait=False``
        (nl_lj_virial_enqueue) a list whose build failed gives 8 NaN.  The first call allocates scratch: make it before
        a graph capture.  After a slab build under set_local_ids: this rank's share (a pair that crosses a cut counts 1/2
        on either side, so n_in may be a half-integer); the ranks' 8 doubles add up to the global box's."""
        return self._consume("nl_lj_virial", q, (epsilon, sigma, rc_force), wait, out, totals=True)

    def lj_virial_typed(self, q, wait=True, out=None):
        """lj_virial with the parameters of set_lj_type_params, per pair of types (nl_lj_virial_typed); ``wait=False``:
        nl_lj_virial_typed_enqueue."""
        return self._consume("nl_lj_virial_typed", q, (), wait, out, totals=True)

    # ------------------------------------------------------------------ tabulated pair potentials
    def set_pair_table(self, F, U, r_min, r_max):
        """A tabulated pair potential for table_forces and table_virial (nl_set_pair_table): ``F = -U'(r) / r`` and
        ``U`` at the knots ``pair_table.knots(r_min, r_max, nknots)``, uniform in r^2 (``pair_table.sample`` makes them from
        callables).  ``(nknots,)``: one table for every pair; ``(nslots, nknots)``: row ``rdf.slot(a, b, ntypes)`` per pair of
        types of set_type_cutoffs, ntypes taken from nslots.  Synchronous; keeps its device buffer where the table fits."""
        import numpy as np

        F, U = (np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in (F, U))
        if F.shape != U.shape or F.ndim not in (1, 2):
            raise TypeError("F and U must both be (nknots,) or (nslots, nknots)")
        nslots = 1 if F.ndim == 1 else F.shape[0]
        nt = int(round(((8 * nslots + 1) ** 0.5 - 1) / 2))
        if nt * (nt + 1) // 2 != nslots:
            raise TypeError(f"{nslots} rows are not ntypes (ntypes + 1) / 2 for any ntypes")
        ptrs = [m.ctypes.data_as(C.POINTER(C.c_double)) for m in (F, U)]
        check(self._lib.nl_set_pair_table(self._h, nt, int(F.shape[-1]), float(r_min), float(r_max), *ptrs), "nl_set_pair_table")

    def clear_pair_table(self):
        check(self._lib.nl_set_pair_table(self._h, 0, 0, 0.0, 0.0, None, None), "nl_set_pair_table")

    def pair_table(self):
        """``{"ntypes", "nknots", "r_min", "r_max"}`` of the table set (nl_get_pair_table), or None without one."""
        nt, nk, lo, hi = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
        code = self._lib.nl_get_pair_table(self._h, C.byref(nt), C.byref(nk), C.byref(lo), C.byref(hi))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_pair_table")
        return {"ntypes": nt.value, "nknots": nk.value, "r_min": lo.value, "r_max": hi.value}

    def table_forces(self, q, wait=True, out=None):
        """lj_forces with the pair function of set_pair_table (nl_table_forces): ``(n, 4) = {fx, fy, fz, pe_i}``, linear
        interpolation in r^2 between the knots, nothing beyond r_max (within the list's cut-off; less the skin with
        ``wait=False``, nl_table_forces_enqueue).  A pair closer than r_min gives NaN to both its particles."""
        return self._consume("nl_table_forces", q, (), wait, out, totals=False)

    def table_virial(self, q, wait=True, out=None):
        """lj_virial with the pair function of set_pair_table (nl_table_virial; ``wait=False``: nl_table_virial_enqueue):
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}``, n_in the pairs within r_max; 8 NaN where a pair lies below r_min."""
        return self._consume("nl_table_virial", q, (), wait, out, totals=True)

    # ------------------------------------------------------------------ embedded-atom potentials
    def set_eam(self, f, G, r_min, r_max, E, P, rho_max):
        """The density and embedding tables of an embedded-atom potential (nl_set_eam); the pair part is the table of
        set_pair_table, which must be set as well (zeros for a model without one).  ``f = f_b(r)`` and ``G = -f_b'(r) / r`` at
        the knots ``pair_table.knots(r_min, r_max, nknots_d)``, ``E = F_a(rho)`` and ``P = F_a'(rho)`` at
        ``rho_k = k rho_max / (nknots_e - 1)`` (``eam.sample`` makes all four from callables).  ``(nknots,)``: one type;
        ``(ntypes, nknots)``: one row per type of set_type_cutoffs.  Synchronous; keeps its device buffer where the tables fit."""
        import numpy as np

        f, G, E, P = (np.ascontiguousarray(np.atleast_2d(np.asarray(m, dtype=np.float64))) for m in (f, G, E, P))
        if f.shape != G.shape or E.shape != P.shape or f.ndim != 2 or E.ndim != 2 or f.shape[0] != E.shape[0]:
            raise TypeError("f, G must both be (ntypes, nknots_d) and E, P both (ntypes, nknots_e)")
        ptr = lambda m: m.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        check(self._lib.nl_set_eam(self._h, int(f.shape[0]), int(f.shape[1]), float(r_min), float(r_max), ptr(f), ptr(G), int(E.shape[1]),
                                   float(rho_max), ptr(E), ptr(P)), "nl_set_eam")

    def clear_eam(self):
        check(self._lib.nl_set_eam(self._h, 0, 0, 0.0, 0.0, None, None, 0, 0.0, None, None), "nl_set_eam")

    def eam(self):
        """``{"ntypes", "nknots_d", "r_min", "r_max", "nknots_e", "rho_max", "lds_density", "lds_forces"}`` of the tables set
        (nl_get_eam), or None without them.  lds_*: the density pass, and the forces and totals, read their tables from LDS."""
        nt, nd, ne, l1, l2 = (C.c_int32() for _ in range(5))
        lo, hi, rm = C.c_double(), C.c_double(), C.c_double()
        code = self._lib.nl_get_eam(self._h, C.byref(nt), C.byref(nd), C.byref(lo), C.byref(hi), C.byref(ne), C.byref(rm), C.byref(l1), C.byref(l2))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_eam")
        return {"ntypes": nt.value, "nknots_d": nd.value, "r_min": lo.value, "r_max": hi.value, "nknots_e": ne.value, "rho_max": rm.value,
                "lds_density": bool(l1.value), "lds_forces": bool(l2.value)}

    def eam_forces(self, q, wait=True, out=None):
        """Embedded-atom forces and per-particle energies (nl_eam_forces; ``wait=False``: nl_eam_forces_enqueue):
        ``(n, 4) = {fx, fy, fz, pe_i}``, pe_i = half the pair energies of i + F(rho_i), so that ``pe.sum()`` is the energy.
        Three passes over the list of the last build: densities, embedding, forces.  A density outside [0, rho_max] or a
        pair below r_min gives NaN.  The first call allocates scratch: make it before a graph capture.  Whole builds only."""
        return self._consume("nl_eam_forces", q, (), wait, out, totals=False)

    def eam_virial(self, q, wait=True, out=None):
        """The totals that belong to eam_forces (nl_eam_virial; ``wait=False``: nl_eam_virial_enqueue):
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}``, U the pair energies plus every F(rho_i).  Bit for bit reproducible
        after a full-list build; after a half-list build the densities are summed by atomics and the totals follow them."""
        return self._consume("nl_eam_virial", q, (), wait, out, totals=True)

    def eam_density(self):
        """``(rho, fp)``: rho_i and F'(rho_i) of the last eam_forces / eam_virial call (nl_eam_get_density), copies of
        ``(n,)`` in the list's dtype, taken on the current stream."""
        rho, fp, n = C.c_void_p(), C.c_void_p(), C.c_int32()
        check(self._lib.nl_eam_get_density(self._h, C.byref(rho), C.byref(fp), C.byref(n)), "nl_eam_get_density")
        ts = "<f4" if self.dtype == torch.float32 else "<f8"
        return tuple(_as_tensor(p.value, (n.value,), ts, self, self.device).clone() for p in (rho, fp))

    # ------------------------------------------------------------------ Stillinger-Weber three-body potentials
    def set_sw(self, g, G, r_min, r_max, lam, cos0):
        """The radial tables and angular parameters of a three-body potential (nl_set_sw); the pair part is the table of
        set_pair_table, which must be set as well (zeros for a model without one).  ``g = g_ab(r)`` and ``G = -g_ab'(r) / r`` at
        the knots ``pair_table.knots(r_min, r_max, nknots)`` (``sw.sample`` makes them from callables): ``(nknots,)`` for one
        type, ``(ntypes^2, nknots)`` with row ``a ntypes + b`` for centre type a and end type b.  ``lam`` and ``cos0``:
        ``(ntypes, ntypes, ntypes)`` as ``sw.angular`` returns them (scalars for one type).  Synchronous; keeps its device
        buffer where the tables fit."""
        import numpy as np

        g, G = (np.ascontiguousarray(np.atleast_2d(np.asarray(m, dtype=np.float64))) for m in (g, G))
        lam, cos0 = (np.ascontiguousarray(np.asarray(m, dtype=np.float64)).reshape(-1) for m in (lam, cos0))
        nt = int(round(g.shape[0] ** 0.5))
        if g.shape != G.shape or g.ndim != 2 or nt * nt != g.shape[0] or lam.shape != (nt ** 3,) or cos0.shape != (nt ** 3,):
            raise TypeError("g, G must both be (ntypes^2, nknots) and lam, cos0 both hold ntypes^3 values")
        ptr = lambda m: m.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        check(self._lib.nl_set_sw(self._h, nt, int(g.shape[1]), float(r_min), float(r_max), ptr(g), ptr(G), ptr(lam), ptr(cos0)), "nl_set_sw")

    def clear_sw(self):
        check(self._lib.nl_set_sw(self._h, 0, 0, 0.0, 0.0, None, None, None, None), "nl_set_sw")

    def sw(self):
        """``{"ntypes", "nknots", "r_min", "r_max", "lds"}`` of the tables set (nl_get_sw), or None without them.  lds: the
        forces and totals read the pair table and the radial tables from LDS."""
        nt, nk, lds = (C.c_int32() for _ in range(3))
        lo, hi = C.c_double(), C.c_double()
        code = self._lib.nl_get_sw(self._h, C.byref(nt), C.byref(nk), C.byref(lo), C.byref(hi), C.byref(lds))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_sw")
        return {"ntypes": nt.value, "nknots": nk.value, "r_min": lo.value, "r_max": hi.value, "lds": bool(lds.value)}

    def sw_forces(self, q, wait=True, out=None):
        """Stillinger-Weber forces and per-particle energies (nl_sw_forces; ``wait=False``: nl_sw_forces_enqueue):
        ``(n, 4) = {fx, fy, fz, pe_i}``, pe_i = half the pair energies of i + a third of every triple i is part of, so that
        ``pe.sum()`` is the energy.  Full lists of whole builds only.  A centre with more than 64 partners within r_max of the
        radial tables, or one closer than their r_min, gives NaN to itself and to those partners."""
        return self._consume("nl_sw_forces", q, (), wait, out, totals=False)

    def sw_virial(self, q, wait=True, out=None):
        """The totals that belong to sw_forces (nl_sw_virial; ``wait=False``: nl_sw_virial_enqueue):
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}``, every pair and every triple once, n_in the pairs within the longer of
        the two ranges.  No atomics: bit for bit reproducible.  The first call allocates scratch: make it before a graph capture."""
        return self._consume("nl_sw_virial", q, (), wait, out, totals=True)

    # ------------------------------------------------------------------ Tersoff bond-order potentials
    def set_tersoff(self, u, U, q, Q, r_min, r_max, gamma, c2_over_d2, d2, h, beta, n, p=None, P=None):
        """The radial tables and parameters of a bond-order potential (nl_set_tersoff); the repulsive part is the table of
        set_pair_table, which must be set as well.  ``u, U = -u'/r``, ``q, Q`` and (optionally, lambda_3 != 0) ``p, P`` at the
        knots ``pair_table.knots(r_min, r_max, nknots)`` (``tersoff.sample`` makes them from callables): ``(nknots,)`` for one
        type, ``(ntypes^2, nknots)`` with row ``a ntypes + b`` for centre type a and end type b.  ``gamma, c2_over_d2, d2, h``:
        ``(ntypes,) * 3`` as ``tersoff.angular`` returns them; ``beta, n``: ``(ntypes,) * 2`` as ``tersoff.bond_order`` returns
        them (scalars for one type).  Synchronous; keeps its device buffer where the tables fit."""
        import numpy as np

        if (p is None) != (P is None):
            raise TypeError("p and P are given together or not at all")
        tabs = [np.ascontiguousarray(np.atleast_2d(np.asarray(m, dtype=np.float64))) for m in (u, U, q, Q) + (() if p is None else (p, P))]
        ang = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)).reshape(-1) for m in (gamma, c2_over_d2, d2, h)]
        bo = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)).reshape(-1) for m in (beta, n)]
        nt = int(round(tabs[0].shape[0] ** 0.5))
        if any(t.shape != tabs[0].shape or t.ndim != 2 for t in tabs) or nt * nt != tabs[0].shape[0] or \
                any(a.shape != (nt ** 3,) for a in ang) or any(b.shape != (nt ** 2,) for b in bo):
            raise TypeError("u, U, q, Q (p, P) must all be (ntypes^2, nknots), the angular arrays hold ntypes^3 values, beta and n ntypes^2")
        ptr = lambda m: m.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        radial = [ptr(t) for t in tabs] + ([None, None] if p is None else [])
        check(self._lib.nl_set_tersoff(self._h, nt, int(tabs[0].shape[1]), float(r_min), float(r_max), *radial, *(ptr(a) for a in ang),
                                       *(ptr(b) for b in bo)), "nl_set_tersoff")

    def clear_tersoff(self):
        check(self._lib.nl_set_tersoff(self._h, 0, 0, 0.0, 0.0, *([None] * 12)), "nl_set_tersoff")

    def get_tersoff(self):
        """``{"ntypes", "nknots", "r_min", "r_max", "p", "lds"}`` of the tables set (nl_get_tersoff), or None without them.  p:
        the p tables are set; lds: the forces and totals read the pair table and the radial tables from LDS."""
        nt, nk, hp, lds = (C.c_int32() for _ in range(4))
        lo, hi = C.c_double(), C.c_double()
        code = self._lib.nl_get_tersoff(self._h, C.byref(nt), C.byref(nk), C.byref(lo), C.byref(hi), C.byref(hp), C.byref(lds))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_tersoff")
        return {"ntypes": nt.value, "nknots": nk.value, "r_min": lo.value, "r_max": hi.value, "p": bool(hp.value), "lds": bool(lds.value)}

    def tersoff_forces(self, q, wait=True, out=None):
        """Tersoff forces and per-particle energies (nl_tersoff_forces; ``wait=False``: nl_tersoff_forces_enqueue):
        ``(n, 4) = {fx, fy, fz, pe_i}``, pe_i = half the pair energies of i + a quarter of b u for each end of every ordered bond,
        so that ``pe.sum()`` is the energy.  Full lists of whole builds only.  A centre with more than 64 partners within r_max
        of the radial tables, or one closer than their r_min, gives NaN to itself and to those partners."""
        return self._consume("nl_tersoff_forces", q, (), wait, out, totals=False)

    def tersoff_virial(self, q, wait=True, out=None):
        """The totals that belong to tersoff_forces (nl_tersoff_virial; ``wait=False``: nl_tersoff_virial_enqueue):
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}``, n_in the pairs within the longer of the two ranges.  No atomics: bit
        for bit reproducible.  The first call allocates scratch: make it before a graph capture."""
        return self._consume("nl_tersoff_virial", q, (), wait, out, totals=True)

    # ------------------------------------------------------------------ per-particle charges
    def set_coulomb_table(self, K, C, r_min, r_max, excluded=False):
        """The charge table of coul_forces and coul_virial (nl_set_coulomb_table): ``C = C(r)`` and ``K = -C'(r) / r`` at the
        knots ``pair_table.knots(r_min, r_max, nknots)``, both ``(nknots,)``, the Coulomb constant folded in (the samplers of
        ``md_neighbor_list_amd.coulomb`` make them).  The pair part is the table of set_pair_table, which must be set as well
        (zeros for a model without one).  Synchronous; keeps its device buffer where the table fits.  ``excluded``: the table
        of the pairs that set_exclusions removed is not set here but with set_excluded_coulomb_table (ValueError)."""
        import ctypes  # (C is the table here)

        import numpy as np

        if excluded:
            raise ValueError("the excluded-pair term has methods of its own: set_excluded_coulomb_table, coul_excl_forces (excluded=False here)")
        K, C = (np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in (K, C))
        if K.shape != C.shape or K.ndim != 1:
            raise TypeError("K and C must both be (nknots,)")
        ptrs = [m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for m in (K, C)]
        check(self._lib.nl_set_coulomb_table(self._h, 0, int(K.shape[0]), float(r_min), float(r_max), *ptrs), "nl_set_coulomb_table")

    def clear_coulomb_table(self, excluded=False):
        if excluded:
            raise ValueError("the excluded-pair term has methods of its own: set_excluded_coulomb_table, coul_excl_forces (excluded=False here)")
        check(self._lib.nl_set_coulomb_table(self._h, 0, 0, 0.0, 0.0, None, None), "nl_set_coulomb_table")

    def coulomb_table_info(self, excluded=False):
        """``{"nknots", "r_min", "r_max", "lds"}`` of the charge table (nl_get_coulomb_table), or None without one.  lds: the
        calls read the pair table and the charge table from LDS."""
        if excluded:
            raise ValueError("the excluded-pair term has methods of its own: set_excluded_coulomb_table, coul_excl_forces (excluded=False here)")
        nk, lds = C.c_int32(), C.c_int32()
        lo, hi = C.c_double(), C.c_double()
        code = self._lib.nl_get_coulomb_table(self._h, 0, C.byref(nk), C.byref(lo), C.byref(hi), C.byref(lds))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_coulomb_table")
        return {"nknots": nk.value, "r_min": lo.value, "r_max": hi.value, "lds": bool(lds.value)}

    def set_charges(self, t):
        """The charges coul_forces and coul_virial read unless they are given others: a contiguous ``(n,)`` device tensor of
        the handle's dtype, one charge per row of the positions (after a slab build under set_local_ids the ghosts'
        included).  A reference is kept, nothing is copied: the tensor may be updated in place, and is permuted with
        ``resort`` like any other per-particle array.  None forgets it."""
        if t is not None:
            self._check_charges(t)
        self._charges = t

    def _check_charges(self, t):
        if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != self.dtype or t.dim() != 1
                or not t.is_contiguous()):
            raise TypeError("charges must be a contiguous (n,) device tensor of the list's dtype")

    def _charge_ptr(self, charges):
        t = self._charges if charges is None else charges
        if t is None:
            return C.c_void_p(None)  # (nl_coul_*: NL_ERR_ARG)
        self._check_charges(t)
        if t.shape[0] != self._n:
            raise ValueError("charges must hold one value per particle of the list's build")
        return C.c_void_p(t.data_ptr())

    def coul_forces(self, q, wait=True, out=None, charges=None):
        """table_forces with the charge term (nl_coul_forces; ``wait=False``: nl_coul_forces_enqueue):
        ``(n, 4) = {fx, fy, fz, pe_i}`` of ``E = sum_pairs [phi(r) + q_i q_j C(r)]``, phi the table of set_pair_table, C the
        table of set_coulomb_table, the charges those of set_charges or ``charges``.  Both r_max within the list's cut-off
        (less the skin with ``wait=False``).  A pair closer than either r_min gives NaN to both its particles."""
        return self._consume("nl_coul_forces", q, (self._charge_ptr(charges),), wait, out, totals=False)

    def coul_virial(self, q, wait=True, out=None, charges=None):
        """The totals that belong to coul_forces (nl_coul_virial; ``wait=False``: nl_coul_virial_enqueue):
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}``, n_in the pairs within the longer of the two ranges; the same for a
        half and a full list, bit for bit reproducible.  The first call allocates scratch: make it before a graph capture."""
        return self._consume("nl_coul_virial", q, (self._charge_ptr(charges),), wait, out, totals=True)

    # ------------------------------------------------------------------ the excluded-pair term of the charges
    def set_excluded_coulomb_table(self, K, C, r_min, r_max):
        """The table of coul_excl_forces and coul_excl_virial (nl_set_coul_excl_table): ``C = C(r)`` and ``K = -C'(r) / r`` at
        the knots ``pair_table.knots(r_min, r_max, nknots)``, both ``(nknots,)``, sign and Coulomb constant folded in
        (``coulomb.ewald_excluded`` makes Ewald's ``-erf(alpha r) / r``).  Every excluded pair must lie in [r_min, r_max): one
        outside has no value and gives NaN.  Synchronous; keeps its device buffer where the table fits; no pair table needed."""
        import ctypes  # (C is the table here)

        import numpy as np

        K, C = (np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in (K, C))
        if K.shape != C.shape or K.ndim != 1:
            raise TypeError("K and C must both be (nknots,)")
        ptrs = [m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for m in (K, C)]
        check(self._lib.nl_set_coul_excl_table(self._h, int(K.shape[0]), float(r_min), float(r_max), *ptrs), "nl_set_coul_excl_table")

    def clear_excluded_coulomb_table(self):
        check(self._lib.nl_set_coul_excl_table(self._h, 0, 0.0, 0.0, None, None), "nl_set_coul_excl_table")

    def excluded_coulomb_table_info(self):
        """``{"nknots", "r_min", "r_max", "lds"}`` of the excluded-pair table (nl_get_coul_excl_table), or None without one.
        lds: the calls read the table from LDS."""
        nk, lds = C.c_int32(), C.c_int32()
        lo, hi = C.c_double(), C.c_double()
        code = self._lib.nl_get_coul_excl_table(self._h, C.byref(nk), C.byref(lo), C.byref(hi), C.byref(lds))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_coul_excl_table")
        return {"nknots": nk.value, "r_min": lo.value, "r_max": hi.value, "lds": bool(lds.value)}

    def coul_excl_forces(self, q, wait=True, out=None, charges=None, add=False):
        """The excluded-pair term (nl_coul_excl_forces; ``wait=False``: nl_coul_excl_forces_enqueue):
        ``(n, 4) = {fx, fy, fz, pe_i}`` of ``E = sum q_i q_j C(r)`` over the pairs of set_exclusions at their nearest image, C
        the table of set_excluded_coulomb_table, the charges those of set_charges or ``charges``.  No cut-off.  ``add``: the
        rows are added to ``out`` (required then) instead of written, so ``coul_excl_forces(q, out=coul_forces(q), add=True)``
        is the complete real-space force.  Whole single-device builds only; no atomics, bit for bit reproducible."""
        if add and out is None:
            raise ValueError("add=True adds to out, which must be given")
        return self._consume("nl_coul_excl_forces", q, (self._charge_ptr(charges),), wait, out, totals=False, tail=(1 if add else 0,))

    def coul_excl_virial(self, q, wait=True, out=None, charges=None):
        """The totals that belong to coul_excl_forces (nl_coul_excl_virial; ``wait=False``: nl_coul_excl_virial_enqueue):
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}``, every excluded pair once, n_in their number; 8 NaN where a pair
        lies outside the table.  The first call allocates scratch (lj_virial's): make it before a graph capture."""
        return self._consume("nl_coul_excl_virial", q, (self._charge_ptr(charges),), wait, out, totals=True)

    # ------------------------------------------------------------------ the DPD pair thermostat
    def set_dpd(self, A, gamma, sigma, r_min, r_max, dt, seed=0):
        """The weight table and the parameters of dpd_forces and dpd_virial (nl_set_dpd): ``A = w(r) / r`` at the knots
        ``pair_table.knots(r_min, r_max, nknots)``, ``(nknots,)`` (``dpd.weight`` makes it); ``gamma`` and ``sigma`` scalars, or
        ``(nslots,)`` with the entry ``rdf.slot(a, b, ntypes)`` per pair of types of set_type_cutoffs, ntypes taken from nslots
        (``dpd.sigma_for(gamma, kT)`` is the sigma of a temperature); ``dt`` the time step the noise is scaled by, ``seed``
        any 64-bit integer.  The pair part is the table of set_pair_table, which must be set as well (zeros for a pure
        thermostat).  Synchronous; keeps its device buffer where the state fits, so a captured graph reads the new values."""
        import numpy as np

        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        g, s = (np.ascontiguousarray(np.atleast_1d(np.asarray(m, dtype=np.float64))) for m in (gamma, sigma))
        if A.ndim != 1 or g.ndim != 1 or g.shape != s.shape:
            raise TypeError("A must be (nknots,), gamma and sigma scalars or both (nslots,)")
        nslots = g.shape[0]
        nt = int(round(((8 * nslots + 1) ** 0.5 - 1) / 2))
        if nt * (nt + 1) // 2 != nslots:
            raise TypeError(f"{nslots} slots are not ntypes (ntypes + 1) / 2 for any ntypes")
        ptrs = [m.ctypes.data_as(C.POINTER(C.c_double)) for m in (A, g, s)]
        check(self._lib.nl_set_dpd(self._h, nt, int(A.shape[0]), float(r_min), float(r_max), *ptrs, float(dt),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF), "nl_set_dpd")

    def clear_dpd(self):
        check(self._lib.nl_set_dpd(self._h, 0, 0, 0.0, 0.0, None, None, None, 0.0, 0), "nl_set_dpd")

    def dpd_info(self):
        """``{"ntypes", "nknots", "r_min", "r_max", "dt", "seed", "lds"}`` of set_dpd (nl_get_dpd), or None while nothing is
        set.  lds: the calls read the pair table, the weight table and the parameters from LDS."""
        nt, nk, lds = C.c_int32(), C.c_int32(), C.c_int32()
        lo, hi, dt, seed = C.c_double(), C.c_double(), C.c_double(), C.c_uint64()
        code = self._lib.nl_get_dpd(self._h, C.byref(nt), C.byref(nk), C.byref(lo), C.byref(hi), C.byref(dt), C.byref(seed), C.byref(lds))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_dpd")
        return {"ntypes": nt.value, "nknots": nk.value, "r_min": lo.value, "r_max": hi.value, "dt": dt.value, "seed": seed.value,
                "lds": bool(lds.value)}

    def _dpd_args(self, v, step, wait):
        """(v pointer, v stride, step pointer) of the DPD calls and what keeps the step word alive.  v: ``(n, 3)`` or
        ``(n, 4)`` of the list's dtype; step: a one-element int64 device tensor (the 64 bits are the counter), or, with
        ``wait=True`` only, a Python int, which is copied to the device for the call."""
        if v is None:
            vp, vs = C.c_void_p(None), 3  # (nl_dpd_*: NL_ERR_ARG)
        else:
            if (not isinstance(v, torch.Tensor) or v.device.type != "cuda" or v.dtype != self.dtype or v.dim() != 2
                    or not v.is_contiguous()):
                raise TypeError("v must be a contiguous (n, 3) or (n, 4) device tensor of the list's dtype")
            if v.shape[0] != self._n:
                raise ValueError("v must hold one row per particle of the list's build")
            vp, vs = C.c_void_p(v.data_ptr()), int(v.shape[1])
        if step is None:
            return (vp, C.c_int32(vs), C.c_void_p(None)), None
        if not isinstance(step, torch.Tensor):
            if not wait:
                raise TypeError("with wait=False the step is a one-element int64 device tensor: nothing is copied from the host")
            u = int(step) & 0xFFFFFFFFFFFFFFFF
            step = torch.tensor([u - (1 << 64) if u >= (1 << 63) else u], dtype=torch.int64, device=self.device)
        if step.device.type != "cuda" or step.dtype != torch.int64 or step.numel() != 1:
            raise TypeError("step must be a one-element int64 device tensor")
        return (vp, C.c_int32(vs), C.c_void_p(step.data_ptr())), step

    def dpd_forces(self, q, v, step, wait=True, out=None):
        """table_forces with the DPD pair term (nl_dpd_forces; ``wait=False``: nl_dpd_forces_enqueue):
        ``(n, 4) = {fx, fy, fz, pe_i}`` of ``F_ij = fr_phi d + [-gamma w^2 (e . v_ij) + sigma w xi_ij / sqrt(dt)] e``, phi the
        table of set_pair_table, the rest that of set_dpd, ``v`` the velocities and ``step`` the counter of the noise, read
        on the device: the caller advances it in stream order, and the same step gives the same noise.  Whole single-device
        builds only.  After ``resort`` (q and v permuted alike) a physical pair draws another number; the statistics stay."""
        # (keep: the step word of a Python int, an allocation of this stream, which orders its reuse behind the kernel)
        args, keep = self._dpd_args(v, step, wait)
        return self._consume("nl_dpd_forces", q, args, wait, out, totals=False)

    def dpd_virial(self, q, v, step, wait=True, out=None):
        """The totals that belong to dpd_forces (nl_dpd_virial; ``wait=False``: nl_dpd_virial_enqueue):
        ``{W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}``, W from the whole pair force, U of phi alone, n_in the pairs within
        the longer of the two ranges; bit for bit reproducible for the same positions, velocities and step.  The first call
        allocates scratch (lj_virial's): make it before a graph capture."""
        args, keep = self._dpd_args(v, step, wait)
        return self._consume("nl_dpd_virial", q, args, wait, out, totals=True)

    def pair_histogram(self, q, r_max, nbins, typed=False, wait=True, out=None):
        """Pair-distance histogram of the list of the last build (nl_pair_histogram): every stored pair once, half or
        full list, in ``nbins`` bins uniform in r up to ``r_max`` (within the list's cut-offs; less the skin with
        ``wait=False``, nl_pair_histogram_enqueue).  Returns a contiguous int64 device tensor ``(nbins,)``, or with
        ``typed`` (nl_pair_histogram_typed) ``(ntypes (ntypes + 1) / 2, nbins)`` with the row ``rdf.slot(a, b, ntypes)`` per
        pair of types of set_type_cutoffs.  New and zeroed when ``out`` is None; otherwise the counts are added to ``out``,
        so frames accumulate.  Exact integer counts, the same for both list kinds; allocates nothing: it can be captured.
        After a slab build under set_local_ids: this rank's share in whole pairs (a pair that crosses a cut is counted by
        exactly one of its two ranks); the ranks' counters add up to the global box's, bit for bit."""
        n = self._check_q(q, None)
        if n != self._n:
            raise ValueError("q must hold the particles the list was built from")
        nbins = int(nbins)
        if typed:
            nt = self._get_types()[2]
            shape = (nt * (nt + 1) // 2, nbins)
        else:
            shape = (nbins,)
        o = torch.zeros(shape, dtype=torch.int64, device=self.device) if out is None else out
        if tuple(o.shape) != shape or o.dtype != torch.int64 or not o.is_contiguous() or o.device != q.device:
            raise TypeError(f"out must be a contiguous int64 tensor of shape {shape} on the list's device")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        name = "nl_pair_histogram" + ("_typed" if typed else "") + ("" if wait else "_enqueue")
        check(getattr(self._lib, name)(self._h, q.data_ptr(), q.shape[1], float(r_max), nbins, o.data_ptr(), stream), name)
        return o

    def rdf(self, hist, r_max, frames=1, types=None):
        """``(r_mid, g)`` from a histogram of pair_histogram (md_neighbor_list_amd.rdf.rdf) with the volume of the box and
        the particle counts of the last build filled in.  ``hist`` ``(nbins,)``: g(r) of all particles.  ``hist``
        ``(nslots, nbins)`` and ``types=(a, b)``: g_ab(r), the counts of a and b taken from the type table.  Raises
        ValueError unless all three axes are periodic (an open axis has no bulk density to normalise by)."""
        import numpy as np

        from . import rdf as _rdf

        if self.periodic_mask() != 7:
            raise ValueError("rdf() needs a box periodic on all three axes")
        if self._n_rows != self._n:
            raise ValueError("rdf() needs the global counts: sum the ranks' histograms of a slab build and call rdf.rdf")
        Lx, Ly, Lz = self.box[:3]
        h = hist.detach().cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
        if types is None:
            if h.ndim != 1:
                raise ValueError("a typed histogram needs types=(a, b)")
            return _rdf.rdf(h, r_max, Lx * Ly * Lz, self._n, frames=frames)
        a, b = (int(t) for t in types)
        nt = self._get_types()[2]
        if h.ndim != 2 or h.shape[0] != _rdf.nslots(nt):
            raise ValueError(f"types=(a, b) picks a row of a typed histogram of {_rdf.nslots(nt)} rows")
        counts = torch.bincount(self.types().to(torch.int64), minlength=nt).cpu()
        return _rdf.rdf(h[_rdf.slot(a, b, nt)], r_max, Lx * Ly * Lz, int(counts[a]), None if a == b else int(counts[b]),
                        frames=frames)

    # ------------------------------------------------------------------ Steinhardt order parameters
    def set_steinhardt(self, l, r_max, w=True):
        """The degree ``l`` (1 .. 12) and the neighbour range ``r_max`` of steinhardt() (nl_set_steinhardt).  ``w``: True
        uploads ``steinhardt.wigner3j_table(l)`` for the w_l columns, False leaves them NaN, an array of ``(2 l + 1, 2 l + 1)``
        is taken as the table.  Synchronous; keeps the list."""
        import numpy as np

        from . import steinhardt as _st

        l = int(l)
        if w is True:
            w = _st.wigner3j_table(l) if 1 <= l <= _st.MAX_L else None
        ptr = None
        if w is not None and w is not False:
            w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
            if w.shape != (2 * l + 1, 2 * l + 1):
                raise TypeError("w must be (2 l + 1, 2 l + 1)")
            ptr = w.ctypes.data_as(C.POINTER(C.c_double))
        check(self._lib.nl_set_steinhardt(self._h, l, float(r_max), ptr), "nl_set_steinhardt")

    def clear_steinhardt(self):
        check(self._lib.nl_set_steinhardt(self._h, 0, 0.0, None), "nl_set_steinhardt")

    def steinhardt_info(self):
        """``{"l", "r_max", "w"}`` of the setting (nl_get_steinhardt), or None without one."""
        l, w, r = C.c_int32(), C.c_int32(), C.c_double()
        code = self._lib.nl_get_steinhardt(self._h, C.byref(l), C.byref(r), C.byref(w))
        if code == _lib.NL_ERR_STATE:
            return None
        check(code, "nl_get_steinhardt")
        return {"l": l.value, "r_max": r.value, "w": bool(w.value)}

    def steinhardt(self, q, average=False, wait=True, out=None):
        """Steinhardt order parameters of every particle over its neighbours within r_max (nl_steinhardt; ``wait=False``:
        nl_steinhardt_enqueue): ``(n, 4) = {q_l, w_l, averaged q_l, averaged w_l}`` in the list's dtype, w_l normalised, the
        averaged forms those of Lechner and Dellago (NaN unless ``average``).  A particle without a neighbour gives NaN.
        Full lists of whole builds only.  The first call allocates scratch: make it before a graph capture."""
        n = self._check_q(q, None)
        if n != self._n:
            raise ValueError("q must hold the particles the list was built from")
        rows = self._n_rows
        o = torch.empty((rows, 4), dtype=self.dtype, device=self.device) if out is None else out
        if o.shape != (rows, 4) or o.dtype != self.dtype or not o.is_contiguous():
            raise TypeError("out must be a contiguous (n_rows, 4) tensor of the list's dtype")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        name = "nl_steinhardt" + ("" if wait else "_enqueue")
        check(getattr(self._lib, name)(self._h, q.data_ptr(), q.shape[1], 1 if average else 0, o.data_ptr(), stream), name)
        return o

    def steinhardt_qlm(self):
        """``(qlm, count)`` of the last steinhardt() call (nl_steinhardt_get_qlm): the un-averaged q_lm as a complex
        ``(n, l + 1)`` tensor (m = 0 .. l) and N_b as int32 ``(n,)``, copies taken on the current stream."""
        p, c, n, l = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        check(self._lib.nl_steinhardt_get_qlm(self._h, C.byref(p), C.byref(c), C.byref(n), C.byref(l)), "nl_steinhardt_get_qlm")
        ts = "<f4" if self.dtype == torch.float32 else "<f8"
        qlm = _as_tensor(p.value, (n.value, l.value + 1, 2), ts, self, self.device).clone()
        return torch.view_as_complex(qlm), _as_tensor(c.value, (n.value,), "<i4", self, self.device).clone()

    # ------------------------------------------------------------------ clusters and solid-like particles
    def _int32_rows(self, t, what, rows):
        if not isinstance(t, torch.Tensor) or t.shape != (rows,) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device:
            raise TypeError(f"{what} must be a contiguous int32 tensor of ({rows},) on the list's device")
        return t

    def clusters(self, q, r_max, member=None, min_member=1, wait=True, sizes=True, summary=True):
        """Connected components of the graph of the stored pairs within ``r_max`` (nl_clusters; ``wait=False``:
        nl_clusters_enqueue).  ``member``: None, everybody; or an int32 ``(n,)`` device tensor, particle i taking part iff
        ``member[i] >= min_member`` -- a 0/1 mask, a type array, or the counts of solid_bonds().  Returns
        ``(labels, sizes, summary)``: ``labels`` int32 ``(n,)``, the smallest particle index of the particle's cluster, -1 for
        a non-member; ``sizes`` int32 ``(n,)``, the size of that cluster, 0 for a non-member; ``summary`` int64 ``(4,)`` =
        ``{members, clusters, size of the largest cluster, its label}``.  ``sizes`` / ``summary``: True for a new tensor,
        a tensor to write into, or False for None.  Exact, and the same bytes for every call, build and list kind; half
        and full lists of whole builds.  With ``summary`` and without ``sizes`` the first call allocates scratch."""
        n = self._check_q(q, None)
        if n != self._n:
            raise ValueError("q must hold the particles the list was built from")
        rows = self._n_rows
        labels = torch.empty(rows, dtype=torch.int32, device=self.device)
        if sizes is True:
            sizes = torch.empty(rows, dtype=torch.int32, device=self.device)
        sizes = None if sizes is None or sizes is False else self._int32_rows(sizes, "sizes", rows)
        if summary is True:
            summary = torch.empty(4, dtype=torch.int64, device=self.device)
        elif summary is None or summary is False:
            summary = None
        elif (not isinstance(summary, torch.Tensor) or summary.shape != (4,) or summary.dtype != torch.int64
              or not summary.is_contiguous() or summary.device != self.device):
            raise TypeError("summary must be a contiguous int64 tensor of (4,) on the list's device")
        if member is not None:
            self._int32_rows(member, "member", rows)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        name = "nl_clusters" + ("" if wait else "_enqueue")
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        check(getattr(self._lib, name)(self._h, q.data_ptr(), q.shape[1], float(r_max), ptr(member), int(min_member),
                                       labels.data_ptr(), ptr(sizes), ptr(summary), stream), name)
        return labels, sizes, summary

    def solid_bonds(self, q, threshold, wait=True, out=None):
        """The number of solid-like bonds of every particle (nl_solid_bonds; ``wait=False``: nl_solid_bonds_enqueue), int32
        ``(n,)``: the neighbours j of steinhardt()'s setting with ``q_l(i) . q_l(j) > threshold |q_l(i)| |q_l(j)|``, from
        the q_lm the last steinhardt() call left -- call it on this list and these positions first.  Full lists of whole
        builds only; allocates nothing."""
        n = self._check_q(q, None)
        if n != self._n:
            raise ValueError("q must hold the particles the list was built from")
        rows = self._n_rows
        o = torch.empty(rows, dtype=torch.int32, device=self.device) if out is None else self._int32_rows(out, "out", rows)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        name = "nl_solid_bonds" + ("" if wait else "_enqueue")
        check(getattr(self._lib, name)(self._h, q.data_ptr(), q.shape[1], float(threshold), o.data_ptr(), stream), name)
        return o

    # ------------------------------------------------------------------ common neighbour analysis
    def cna(self, q, r_max, adaptive=True, counts=False, summary=True, wait=True):
        """Common neighbour analysis of every particle over its candidates within ``r_max`` (nl_cna; ``wait=False``:
        nl_cna_enqueue).  ``adaptive``: Stukowski's per-particle cut-off on the 12 and 14 nearest candidates (any ``r_max``
        that holds at least 14 candidates of every particle and at most 64), else one fixed cut-off ``r_max``
        (``cna.default_r_max``).  Returns ``(types, counts, summary)``: ``types`` int32 ``(n,)``, 0 other, 1 fcc, 2 hcp, 3 bcc,
        4 icosahedral (``cna.NAMES``); ``counts`` int32 ``(n, 8)`` = ``{N_b, size of the set analysed, n421, n422, n444, n555,
        n666, flags}``; ``summary`` int64 ``(6,)`` = the number of particles of each type and of centres with more than 64
        candidates.  ``counts`` / ``summary``: True for a new tensor, a tensor to write into, or False for None.  Exact;
        full lists of whole builds only; allocates nothing on the handle, so the first call can be captured."""
        n = self._check_q(q, None)
        if n != self._n:
            raise ValueError("q must hold the particles the list was built from")
        rows = self._n_rows
        types = torch.empty(rows, dtype=torch.int32, device=self.device)

        def out(t, shape, dtype, what):
            if t is True:
                return torch.empty(shape, dtype=dtype, device=self.device)
            if t is None or t is False:
                return None
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()
                    or t.device != self.device):
                raise TypeError(f"{what} must be a contiguous {dtype} tensor of {shape} on the list's device")
            return t

        counts = out(counts, (rows, 8), torch.int32, "counts")
        summary = out(summary, (6,), torch.int64, "summary")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        name = "nl_cna" + ("" if wait else "_enqueue")
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        check(getattr(self._lib, name)(self._h, q.data_ptr(), q.shape[1], 1 if adaptive else 0, float(r_max), types.data_ptr(),
                                       ptr(counts), ptr(summary), stream), name)
        return types, counts, summary

    # ------------------------------------------------------------------ periodic re-sorting (SORT_FREQ)
    def cell_order(self):
        """order[s] = input index of the particle at cell-ordered slot s of the last build (nl_get_cell_order; the
        reference's ptcl_id_in_mesh).  View, valid until the next build."""
        ptr, n = C.c_void_p(), C.c_int32()
        check(self._lib.nl_get_cell_order(self._h, C.byref(ptr), C.byref(n)), "nl_get_cell_order")
        return _as_tensor(ptr.value, (n.value,), "<i4", self, self.device)

    def resort(self, *arrays):
        """Permutes per-particle device arrays in place into the cell order of the last build (nl_resort): the re-sort
        the reference declares (SORT_FREQ, CopyGather, SortPtclData) and never calls.  Rebuild afterwards."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for t in arrays:
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or not t.is_contiguous() or t.shape[0] != self._n:
                raise TypeError("resort() takes contiguous device tensors with one leading entry per particle")
            check(self._lib.nl_resort(self._h, t.data_ptr(), t.element_size() * (t.numel() // max(t.shape[0], 1)), stream), "nl_resort")

    # ------------------------------------------------------------------ introspection
    def sorted_state(self):
        """(cell_start, sorted_row) of the last build -- for tests of the hash/sort stage.  In a fine-row build
        (build_info()['fine_rows'] > 0) the table has 4 entries per cell: [(row * mx + cx) * 4 + quarter], the four
        fine rows (quarters of the cell along z) of every row of x-cells."""
        cs, sp, sr, ncl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        check(self._lib.nl_get_sorted(self._h, C.byref(cs), C.byref(sp), C.byref(sr), C.byref(ncl)), "nl_get_sorted")
        entries = ncl.value * (4 if self.build_info()["fine_rows"] else 1) + 1
        return (_as_tensor(cs.value, (entries,), "<i4", self, self.device),
                _as_tensor(sr.value, (self._n,), "<i4", self, self.device))

    def profile_stages(self, q, reps=10):
        """Average device milliseconds per pipeline stage (HIP events on the launch stream)."""
        n = self._check_q(q, None)
        ms = (C.c_double * _lib.NL_NUM_STAGES)()
        check(self._lib.nl_profile_stages(self._h, q.data_ptr(), q.shape[1], n, int(reps), C.byref(ms)),
              "nl_profile_stages")
        self._n = self._n_rows = n
        return dict(zip(_lib.STAGE_NAMES, (float(v) for v in ms)))


    def build_info(self):
        """{'masks': bool, 'variant': int, 'lds_batch': int, 'cus': int, 'offset_bits': 32 | 64, 'mask_rows': int,
        'fine_rows': 0 | 1 + RowsCfg, 'small_cells': 0 | 1, 'id_classes': 0 | 2 | 4, 'binning': 'two_pass' | 'bucket' |
        'atomic', 'reach_cull': bool} of the last build (masks: the list was expanded from hit masks; mask_rows > 1: dense
        build; fine_rows: the fine-row search of nl_rows.hpp; id_classes: the half-list search by id class, NL_IDCLASS;
        binning: two passes over rows of x-cells, one pass into row buckets, or atomic ranks into the cell histogram --
        NL_BINNING=1 and meshes beyond the row tables; reach_cull: the id-class search dropped the partners no particle of
        the cell can reach before it searched, NL_CULL)."""
        info = (C.c_int32 * 8)()
        check(self._lib.nl_get_build_info(self._h, C.byref(info)), "nl_get_build_info")
        return {"masks": bool(info[0]), "variant": int(info[1]), "lds_batch": int(info[2]), "cus": int(info[3]),
                "offset_bits": int(info[4]), "mask_rows": int(info[5]), "fine_rows": int(info[6]),
                "small_cells": int(info[7]) & 0xFF, "id_classes": int(info[7]) >> 8 & 0xFF,
                "binning": ("two_pass", "bucket", "atomic")[int(info[7]) >> 16 & 3],
                "reach_cull": bool(int(info[7]) >> 18 & 1)}

    def build_stats(self):
        """{'row_overflow_reruns', 'list_reruns', 'cap_row', 'list_launched'}: builds of this handle run again (a row
        past its bucket; cells for the list kernels while those were left out) and how the last build ran."""
        st = (C.c_int64 * 4)()
        check(self._lib.nl_get_build_stats(self._h, C.byref(st)), "nl_get_build_stats")
        return {"row_overflow_reruns": int(st[0]), "list_reruns": int(st[1]), "cap_row": int(st[2]),
                "list_launched": bool(st[3])}

    def profile_last_build(self, reps=10):
        """Same for the last build (also a slab build); its position/id tensors are kept alive by this object.  Not a
        passive timer (nl_profile_last_build): the build is planned again as one whole, ungated build (a begin / finish pair as
        one call; a build that was run again, or an update's, with the two-pass binning and every launch it ran with), run
        ``reps`` times into the handle's own buffers from the positions the tensor holds now, and adopted -- the list,
        ``build_info()`` and ``build_stats()`` afterwards are that build's, and like any build other than an update's it
        makes the next ``update()`` build."""
        ms = (C.c_double * _lib.NL_NUM_STAGES)()
        check(self._lib.nl_profile_last_build(self._h, int(reps), C.byref(ms)), "nl_profile_last_build")
        return dict(zip(_lib.STAGE_NAMES, (float(v) for v in ms)))


def axes_mask(axes) -> int:
    """nl_set_periodic_axes mask of ``axes``: a 3-tuple of bools, a string drawn from "xyz", or a truth value (all
    axes or none)."""
    if isinstance(axes, str):
        if any(c not in "xyz" for c in axes.lower()):
            raise ValueError(f"periodic axes {axes!r}: use letters from 'xyz'")
        return sum(1 << "xyz".index(c) for c in set(axes.lower()))
    if not hasattr(axes, "__len__"):
        return 7 if axes else 0
    axes = tuple(axes)
    if len(axes) != 3:
        raise ValueError(f"periodic axes {axes!r}: a 3-tuple of bools or a string from 'xyz'")
    return sum(1 << d for d in range(3) if axes[d])


def npairs_exceeds_int32(nl) -> bool:
    """True when the last list is too long for int32 offsets (then the int32 key_pointer accessor is not asked for)."""
    n = C.c_int64()
    check(nl._lib.nl_number_of_pairs(nl._h, C.byref(n)), "nl_number_of_pairs")
    return (2 if nl.full_list else 1) * int(n.value) > 2147483647


def device_count() -> int:
    c = C.c_int()
    check(_lib.load().nl_device_count(C.byref(c)))
    return int(c.value)
