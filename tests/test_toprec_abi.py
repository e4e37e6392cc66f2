"""CPU tests of _writeRecord's device form at the ABI (lx_postprocess_records_dev, lx_iterate_matches_dev_top): the symbols and the
binding's wrappers exist, bad arguments are refused before any device work, and the tests' own yardstick -- the Python restatement of
src/search_algo.hpp:820-882 in tests/toprec_reference.py -- agrees with the host form lx_postprocess_records."""
import ctypes as C

import numpy as np
import pytest

from lambda_amd import capi
from tests import toprec_reference as ref


def test_the_two_symbols_are_exported(lx_lib):
    assert hasattr(lx_lib, "lx_postprocess_records_dev") and hasattr(lx_lib, "lx_iterate_matches_dev_top")
    assert {"lx_postprocess_records_dev", "lx_iterate_matches_dev_top"} <= set(capi.EXPORTED_SYMBOLS)
    assert lx_lib.lx_abi_version() == 3
    assert callable(capi.postprocess_records_dev) and callable(capi.Handle.iterate_matches_dev_top)


def test_bad_arguments_are_refused_without_a_device(lx_lib):
    m = np.zeros(4, dtype=capi.BLAST_MATCH_DTYPE)
    st, n, res = capi.RecordStats(), C.c_uint64(7), C.c_void_p()
    params = capi.SearchParams(1e-2, -1, 0, 1000, 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, capi.karlin_params(62))
    assert lx_lib.lx_postprocess_records_dev(None, capi._ptr(m), 4, 25, C.byref(st), C.byref(n)) == capi.LX_EINVAL
    assert lx_lib.lx_postprocess_records_dev(None, None, 4, 25, C.byref(st), C.byref(n)) == capi.LX_EINVAL
    assert lx_lib.lx_postprocess_records_dev(None, capi._ptr(m), 4, 25, C.byref(st), None) == capi.LX_EINVAL
    assert lx_lib.lx_iterate_matches_dev_top(None, 0, None, 0, C.byref(params), 25, C.byref(st), C.byref(res)) == capi.LX_EINVAL
    assert lx_lib.lx_iterate_matches_dev_top(None, 0, None, 0, C.byref(params), 25, C.byref(st), None) == capi.LX_EINVAL
    assert res.value is None


@pytest.mark.parametrize("max_matches", [0, 1, 25, 2 ** 40])
def test_the_restatement_agrees_with_the_host_form(lx_lib, max_matches):
    rng = np.random.default_rng(5)
    m = np.concatenate([ref.crafted_rows(rng, ref.EDGE_SEGMENTS), ref.crafted_rows(rng, [40, 7, 300], wide=True, qids=[3, 9, 3])])
    want, wst = ref.write_record(m, max_matches)
    got, gst = capi.postprocess_records(m, max_matches)
    assert ref.stats_dict(gst) == wst
    assert np.array_equal(got, want) and got.tobytes() == want.tobytes()
    if max_matches == 25:
        assert wst["hits_duplicate2"] > 1000 and wst["hits_abundant"] > 1000 and wst["qrys_with_hit"] == len(ref.EDGE_SEGMENTS) + 3
