"""Worker of the multi-process cases of tests/test_slab_exclusions.py (gloo, ranks sharing the device; the pattern of
tests/slab_worker.py): nl_make_list_distributed with the same global exclusion table on every rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def keys_of(kp, lst, row_gid=None):
    rows = np.repeat(np.arange(len(kp) - 1, dtype=np.int64), np.diff(kp))
    if row_gid is not None:
        rows = row_gid.astype(np.int64)[rows]
    return (rows << 32) | np.asarray(lst, dtype=np.int64)


def topology(q, rc, box, seed):
    """Pairs in global ids, the same on every rank: a twentieth of the listed pairs of the first configuration, as many
    random pairs (beyond the cut-off, nearly all), a hub with all its partners and 40 strangers, duplicates, both orders."""
    from oracle import pyoracle as po

    n = len(q)
    h = po.build(q, rc, box).canonical()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(h.key_pointer))
    lst = np.asarray(h.sorted_list, dtype=np.int64)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(lst), size=len(lst) // 20, replace=False)
    near = np.stack([rows[pick], lst[pick]], axis=1)
    far = rng.integers(0, n, size=(len(pick), 2))
    far = far[far[:, 0] != far[:, 1]]
    hub = int(np.argmax(np.diff(h.key_pointer)))
    partners = np.union1d(lst[h.key_pointer[hub]:h.key_pointer[hub + 1]], np.setdiff1d(rng.choice(n, 48, replace=False), [hub])[:40])
    assert len(partners) > 32
    star = np.stack([np.full(len(partners), hub, dtype=np.int64), partners], axis=1)
    pairs = np.concatenate([near, far, star, near[: len(near) // 4], near[len(near) // 4: len(near) // 2, ::-1]])
    return pairs[rng.permutation(len(pairs))]


def worker(rank, world, port, case, ret):
    import torch
    import torch.distributed as dist

    from md_neighbor_list_amd import NeighListGPU, inputs, slab
    from md_neighbor_list_amd.dist import DistributedNeighList
    from oracle import pyoracle as po
    from tests.test_exclusions import full_from_half, remove_pairs
    from tests.test_slab_paths import mix_sum

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n, box, rc, dtype, seed, full = case
        q, box = inputs.uniform_box(n, dtype=np.dtype(dtype).type, seed=seed, box=box)
        pairs = topology(q, rc, box, seed + 1)
        nl = NeighListGPU(rc, *box, dtype=torch.float32 if q.dtype == np.float32 else torch.float64, full_list=full)
        nl.Initialize(int(2.2 * n / world) + 8192)
        nl.set_exclusions_global(pairs, n)  # once: the table speaks in global ids, whoever owns them
        dn = DistributedNeighList(nl, rank, world, transport="host")
        rng = np.random.default_rng(5)
        seen = []
        for rnd in range(2):
            if rnd == 1:  # everybody moves by up to 0.45 cells: particles change layer and owner, ghost counts change
                q = q.copy()
                q[:, :3] += rng.uniform(-1.5, 1.5, size=(n, 3)).astype(q.dtype)
                q[:, :3] = np.mod(q[:, :3], np.array(box, dtype=q.dtype))
                q[:, :3] = np.minimum(q[:, :3], np.nextafter(np.array(box, dtype=q.dtype), q.dtype.type(0)))
            dn.scatter(torch.from_numpy(q).cuda(), box, rc)
            owners = slab.z_layer(torch.from_numpy(q), box, rc).numpy()
            for sync in (True, False):
                dn.build(sync=sync)
                nl.synchronize()
                dn.ghosts()
                if full:
                    kp, sl, _cnt = (t.cpu().numpy() for t in nl.full_csr())
                else:
                    kp, sl = nl.key_pointer().cpu().numpy(), nl.sorted_list().cpu().numpy()
                assert len(kp) == dn.n_owned + 1
                cs, ne = nl.list_checksum()
                assert ne == len(sl) == int(kp[-1]) == nl.list_entries()
                assert nl.half_number_of_pairs() == (len(sl) // 2 if full else len(sl))
                mine = keys_of(kp, sl, dn.gid_owned.cpu().numpy())
                gathered = [None] * world
                dist.all_gather_object(gathered, (mine, dn.n_owned, dn.n_ghost_lo, dn.n_ghost_hi, cs))
                if rank == 0:
                    ref = po.build(q, rc, box).canonical()
                    kp_r, lst_r = full_from_half(ref.key_pointer, ref.sorted_list) if full else (ref.key_pointer, ref.sorted_list)
                    cnt_w, kp_w, lst_w = remove_pairs(kp_r, lst_r, pairs)
                    assert 0 < len(lst_w) < len(lst_r), (rnd, len(lst_w), len(lst_r))  # (the table still removes listed pairs)
                    got = np.sort(np.concatenate([g[0] for g in gathered]))
                    assert sum(g[1] for g in gathered) == n
                    assert len(got) == len(lst_w), (rnd, sync, len(got), len(lst_w))
                    assert np.array_equal(got, np.sort(keys_of(kp_w, lst_w))), (rnd, sync)
                    assert sum(g[4] for g in gathered) % 2**64 == mix_sum(np.arange(n), cnt_w.astype(np.int64), lst_w), (rnd, sync)
            seen.append((dn.n_owned, dn.n_ghost_lo, dn.n_ghost_hi, owners))
        g2 = [None] * world
        dist.all_gather_object(g2, [s[:3] for s in seen])
        if rank == 0:
            assert any(a[0] != a[1] for a in g2), g2  # owned and ghost counts did change between the builds
            assert (seen[0][3] != seen[1][3]).any()   # particles changed layer
            ret.put(("ok", 0, g2))
    except Exception as e:  # pragma: no cover
        import traceback

        ret.put(("fail", rank, traceback.format_exc()))
        raise e
    finally:
        dist.destroy_process_group()


def run(world, case, timeout=600):
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(rank, world, port, case, ret)) for rank in range(world)]
    for p in procs:
        p.start()
    try:
        res = ret.get(timeout=timeout)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert res[0] == "ok", res
    return res
