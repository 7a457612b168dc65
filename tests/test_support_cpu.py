"""The shared helpers of ``support.py`` bite: the bitwise comparison sees one ulp in one array of one member, a shape, a
length and (unless told otherwise) NaN against NaN; ``sub_log`` against slices written out by hand; the compiled kernel's
resources are parsed once per source; ``assert_abi`` refuses a name the header does not declare."""
import numpy as np
import pytest

import support as sp
from support import lib


def _snapshot():
    return [(np.arange(4.0) + b, np.eye(4) * (b + 1)) for b in range(3)]


def test_assert_same_sees_one_ulp_in_one_array_of_one_member():
    a, b = _snapshot(), _snapshot()
    sp.assert_same(a, b, "equal")
    assert sp.same(a, b)
    b[2][1][3, 3] = np.nextafter(b[2][1][3, 3], np.inf)
    with pytest.raises(AssertionError, match="member 2 array 1"):
        sp.assert_same(a, b, "one ulp")
    assert not sp.same(a, b) and not sp.same(a, b, equal_nan=True)


def test_assert_same_sees_shapes_and_lengths():
    a, b = _snapshot(), _snapshot()
    b[1] = (b[1][0], b[1][1][:, :3])
    with pytest.raises(AssertionError, match="member 1 array 1 shape"):
        sp.assert_same(a, b, "shape")
    with pytest.raises(AssertionError, match="length 3 != 2"):
        sp.assert_same(a, a[:2], "members")
    with pytest.raises(AssertionError, match="member 0 length 2 != 1"):
        sp.assert_same(a, [m[:1] for m in a], "arrays")
    # one row against the same row repeated: equal after broadcasting, not the same
    assert not sp.same(np.zeros(3), np.zeros((2, 3)))
    # id tables count
    assert sp.same([(np.zeros(2), {4: 0})], [(np.zeros(2), {4: 0})]) and not sp.same([(np.zeros(2), {4: 0})], [(np.zeros(2), {4: 1})])


def test_nan_equals_nan_only_when_asked():
    a, b = _snapshot(), _snapshot()
    a[0][0][1] = b[0][0][1] = np.nan
    with pytest.raises(AssertionError, match="member 0 array 0 values"):
        sp.assert_same(a, b, "nan")
    sp.assert_same(a, b, "nan", equal_nan=True)
    assert not sp.same(a, b) and sp.same(a, b, equal_nan=True)


def test_sub_log_against_slices_written_by_hand():
    poses = np.arange(18.0).reshape(3, 6)
    log = {"ids": np.array([7, 9, 7], np.int32), "poses": poses, "offsets": np.array([0, 2, 2, 3]),
           "has_detections": np.array([True, False, True])}           # widths 2, 0, 1
    whole = sp.sub_log(log, 0, 3)
    assert all(np.array_equal(whole[k], log[k]) for k in log) and set(whole) == set(log)
    tail = sp.sub_log(log, 1, 3)
    assert tail["ids"].tolist() == [7] and np.array_equal(tail["poses"], poses[2:3])
    assert tail["offsets"].tolist() == [0, 0, 1] and tail["has_detections"].tolist() == [False, True]
    empty = sp.sub_log(log, 1, 2)
    assert empty["ids"].size == 0 and empty["poses"].shape == (0, 6)
    assert empty["offsets"].tolist() == [0, 0] and empty["has_detections"].tolist() == [False]
    head = sp.sub_log(log, 0, 1)
    assert head["ids"].tolist() == [7, 9] and head["offsets"].tolist() == [0, 2] and head["has_detections"].tolist() == [True]


def test_kernel_resources_compiles_a_source_once():
    found = sp.kernel_resources("ekf_batch_replicas.hip", r"ekf_replica_poses_kernel")
    assert len(found) == 1, found
    (name, res), = found.items()
    assert "ekf_replica_poses_kernel" in name and set(res) == set(sp.RESOURCE_FIELDS)
    assert [res[k] for k in sp.BUDGET_FIELDS] == [0, 0, 0], res
    assert res["vgpr_count"] > 0 and all(isinstance(v, int) for v in res.values())
    before = sp.compiled_kernels.cache_info()
    assert sp.kernel_resources("ekf_batch_replicas.hip", r"ekf_replica_poses_kernel") == found
    assert sp.kernel_resources("ekf_batch_replicas.hip", r"no_such_kernel") == {}
    assert sp.kernel_resources("ekf_batch_replicas.hip") == found          # (the file's only kernel)
    after = sp.compiled_kernels.cache_info()
    assert after.misses == before.misses and after.hits == before.hits + 3


def test_assert_abi_refuses_a_name_the_header_does_not_declare(lib):
    sp.assert_abi(lib, ("ekf_query_sizes",))
    sp.assert_abi(lib, ("ekf_last_error_string",), returns="const char *")
    with pytest.raises(AssertionError, match="ekf_no_such_call"):
        sp.assert_abi(lib, ("ekf_query_sizes", "ekf_no_such_call"))
    with pytest.raises(AssertionError, match="ekf_last_error_string"):
        sp.assert_abi(lib, ("ekf_last_error_string",))          # (declared, but not as an int)
