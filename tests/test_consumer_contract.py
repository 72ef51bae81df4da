"""The descriptions that tests.consumer_contract works from name the library's entry points and the wrapper's methods as
strings.  A typo there must fail here, on the CPU, and not as a GPU test that never ran."""
from md_neighbor_list_amd import _lib


def _descriptions():
    """Every family's description, from the test module that holds its references and its check."""
    from tests.test_eam import EAM
    from tests.test_pair_table import TABLE
    from tests.test_sw import SW

    return {"table": TABLE, "eam": EAM, "sw": SW}


def test_descriptions_name_real_entry_points():
    """The four entry points are declared with one signature, and the wrapper's methods exist on the class (no handle, no
    library build)."""
    from md_neighbor_list_amd.neighlist import NeighListGPU

    found = _descriptions()
    assert len(found) == 3
    for family, d in found.items():
        assert len(d.entry) == 4 and len(set(d.entry)) == 4, family
        for name in d.entry:
            assert name in _lib.PROTOTYPES, (family, name)
        assert len({repr(_lib.PROTOTYPES[name]) for name in d.entry}) == 1, family  # the same result and argument types
        assert d.entry[1] == d.entry[0] + "_enqueue" and d.entry[3] == d.entry[2] + "_enqueue", family
        for method in (d.forces, d.virial, d.scratch, d.clear, d.info):
            assert callable(getattr(NeighListGPU, method, None)), (family, method)
        assert "nl_" + d.forces == d.entry[0] and "nl_" + d.virial == d.entry[2], family  # the wrapper's call is the entry point
        assert d.scratch in (d.forces, d.virial) and d.kinds, family
