"""Host-side checks of the multi-device group (include/tdoa_mi355x.h, "multi-device group"): the sample runs a member
uploads are tdoa_amd/sharding.py's owned_sample_runs, and tdoa_group_create refuses bad arguments before it asks for a
device, and a device ordinal past tdoa_device_count() the way tdoa_create does -- on a host with or without a GPU."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_owned_runs_are_the_sharding_modules_runs(capi):
    """tdoa_debug_owned_runs against sharding.owned_sample_runs: worlds 1..9, window counts on both sides of W < world
    (the pair-major fallback uploads the whole capture), captures longer than the shortest one by a ragged amount, windows
    that do not tile their block, and adjacent owned windows merged into one run"""
    from tdoa_amd import sharding
    merged = whole = 0
    for world in range(1, 10):
        for wlen in (1000, 997):
            for wpb in (1, 2, 3, 5):
                for spare in (0, 1, 2, 640):                       # samples per block beyond wpb windows
                    n_min = 3 * (wpb * wlen + spare)
                    for extra in (0, 1, 2, 5, 3001, 2 * wlen + 7):  # this capture against the shortest one
                        total = n_min + extra
                        cover = 0
                        for rank in range(world):
                            got = capi.owned_runs(total, n_min, wlen, rank, world)
                            want = sharding.owned_sample_runs(rank, world, total, wlen, n_min)
                            assert got == want, (world, wlen, wpb, spare, extra, rank)
                            merged += any(c > wlen for _, c in got)
                            whole += got == [(0, total)]
                            cover += sum(c for _, c in got)
                        if 3 * wpb >= world:
                            assert cover == 3 * wpb * wlen            # the members' runs partition the windowed samples
    assert merged and whole
    # window longer than a block: one window of n_min / 3 samples per block
    for world in (1, 2, 3, 4):
        for rank in range(world):
            assert capi.owned_runs(90_001, 90_000, 2_000_000, rank, world) == \
                sharding.owned_sample_runs(rank, world, 90_001, 2_000_000, 90_000)
    # a capture too short to window (n_min / 3 == 0)
    assert capi.owned_runs(2, 2, 1000, 0, 1) == sharding.owned_sample_runs(0, 1, 2, 1000, 2) == [(0, 2)]


def test_owned_runs_count_query_and_argument_checks(capi):
    L = capi.load()
    n = C.c_int(-1)
    assert L.tdoa_debug_owned_runs(60_000, 60_000, 10_000, 0, 2, None, None, 0, C.byref(n)) == 0 and n.value == 3
    first, count = (C.c_size_t * 1)(7), (C.c_size_t * 1)(7)
    assert L.tdoa_debug_owned_runs(60_000, 60_000, 10_000, 0, 2, first, count, 1, C.byref(n)) == 0
    assert n.value == 3 and (first[0], count[0]) == (0, 10_000)          # the first run only: room for one
    for args in ((60_000, 60_000, 10_000, 2, 2), (60_000, 60_000, 10_000, -1, 2), (60_000, 60_000, 10_000, 0, 0),
                 (60_000, 60_000, 0, 0, 1), (60_000, 60_001, 10_000, 0, 1)):
        assert L.tdoa_debug_owned_runs(*args, None, None, 0, C.byref(n)) == 1, args
    assert L.tdoa_debug_owned_runs(60_000, 60_000, 10_000, 0, 1, None, None, 1, C.byref(n)) == 1   # room for one, no arrays
    assert L.tdoa_debug_owned_runs(60_000, 60_000, 10_000, 0, 1, None, None, 0, None) == 1
    with pytest.raises(ValueError):
        capi.owned_runs(60_000, 60_000, 10_000, 2, 2)


def test_group_create_checks_arguments_before_devices(capi):
    """TDOA_ERR_INVALID for no members, NULL devices / out and a negative ordinal -- even on a host without a GPU, where
    asking for the device count first would have answered TDOA_ERR_NO_DEVICE -- and *out stays NULL"""
    L = capi.load()
    p = capi.default_params()
    h = C.c_void_p(1234)
    devs = (C.c_int32 * 2)(0, 0)
    assert L.tdoa_group_create(C.byref(p), devs, 0, C.byref(h)) == 1 and not h.value
    h = C.c_void_p(1234)
    assert L.tdoa_group_create(C.byref(p), devs, -3, C.byref(h)) == 1 and not h.value
    h = C.c_void_p(1234)
    assert L.tdoa_group_create(C.byref(p), None, 2, C.byref(h)) == 1 and not h.value
    assert L.tdoa_group_create(C.byref(p), devs, 2, None) == 1
    past = L.tdoa_device_count()
    h = C.c_void_p(1234)
    neg = (C.c_int32 * 3)(past, 0, -1)                      # member 0 past the count, member 2 negative: INVALID first
    assert L.tdoa_group_create(C.byref(p), neg, 3, C.byref(h)) == 1 and not h.value
    assert b"member 2 (device -1)" in L.tdoa_group_last_error(None)
    L.tdoa_group_destroy(None)                              # must be a no-op
    assert L.tdoa_group_member(None, 0) is None
    assert L.tdoa_group_process(None, None) == 1
    assert L.tdoa_group_capture_upload_files(None, 1, None, None) == 1


def test_group_create_refuses_an_ordinal_past_the_device_count_like_tdoa_create(capi):
    import tdoa_amd
    L = capi.load()
    n = L.tdoa_device_count()
    p = capi.default_params()
    p.device = n
    h = C.c_void_p(1234)
    assert L.tdoa_create(C.byref(p), C.byref(h)) == 2 and not h.value
    devs = (C.c_int32 * 2)(0, n) if n > 0 else (C.c_int32 * 1)(n)
    k = len(devs) - 1
    h = C.c_void_p(1234)
    assert L.tdoa_group_create(C.byref(capi.default_params()), devs, len(devs), C.byref(h)) == 2   # TDOA_ERR_NO_DEVICE
    assert not h.value
    assert ("member %d (device %d)" % (k, n)).encode() in L.tdoa_group_last_error(None)
    with pytest.raises(tdoa_amd.TdoaError) as e:
        tdoa_amd.Group(list(devs))
    assert e.value.status == 2 and ("member %d (device %d)" % (k, n)) in str(e.value)
