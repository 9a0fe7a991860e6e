"""GPU: the multi-device group (tdoa_group_*).  Members that share device 0 -- one GPU is what a test box has -- shard the
windows of .dat files as ranks of tdoa_process do and merge on the host: the peaks must be byte-identical to one context's
on the same files, in the window-major layout and in the pair-major fallback, on equal and on ragged captures, and on a
replayed step.  Each member holds exactly the sample runs of its windows; members whose captures disagree are refused
without the output being touched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK, WLEN, MAX_LAG = 30000, 10000, 300
DELAYS = (0, 13, 40)
ST = [(41.18660274289527, -95.96064116595667, 355.69), (41.24669616513154, -96.08366304481238, 329.0),
      (41.32916620016985, -96.03513381562004, 373.18)]
TX = (41.20, -96.00, 400.0)


def _write(tmp_path, oracle, extra=(0, 0, 0)):
    paths = []
    for i, (d, x) in enumerate(zip(DELAYS, extra)):
        path = tmp_path / ("station%d.dat" % i)
        np.asarray(oracle.simulate_delayed_fm(3 * BLOCK + x, d, 77, 10 + i), dtype=np.uint8).tofile(path)
        paths.append(str(path))
    return paths


def _single(paths, window_len):
    import tdoa_amd
    with tdoa_amd.Context(max_lag=MAX_LAG, window_len=window_len) as c:
        for s, p in enumerate(paths):
            c.capture_upload_file(s, p)
        return c.process()


def test_group_of_one_is_the_single_context(tmp_path, oracle):
    import tdoa_amd
    paths = _write(tmp_path, oracle)
    want = _single(paths, WLEN)
    with tdoa_amd.Group([0], max_lag=MAX_LAG, window_len=WLEN) as g:
        assert g.capture_upload_files(paths) == [3 * BLOCK] * 3
        got = g.process()
    assert got.tobytes() == want.tobytes()
    assert (want[:, 0]["lag"] == 13).all() and (want[:, 1]["lag"] == 40).all() and (want[:, 2]["lag"] == 27).all()


@pytest.mark.parametrize("n_members, window_len, extra", [
    (2, WLEN, (0, 0, 0)),                    # window-major: 9 windows over 2 members
    (3, WLEN, (0, 0, 0)),
    (3, WLEN, (0, 1234, 7001)),              # ragged: every capture cut into its own thirds, the grid from the shortest
    (4, BLOCK, (0, 0, 0)),                   # 3 windows, 4 members: the pair-major fallback
    (4, BLOCK, (0, 1234, 7001)),
])
def test_members_sharing_one_device_reproduce_one_context(tmp_path, oracle, n_members, window_len, extra):
    import tdoa_amd
    paths = _write(tmp_path, oracle, extra)
    want = _single(paths, window_len)
    assert (want["abs_corr"] > 0).all()      # every record of the reference is written: a merge that drops one shows
    raw = [np.fromfile(p, dtype=np.uint8) for p in paths]
    with tdoa_amd.Group([0] * n_members, max_lag=MAX_LAG, window_len=window_len) as g:
        ns = g.capture_upload_files(paths)
        assert ns == [3 * BLOCK + x for x in extra]
        got = g.process()
        again = g.process()                  # the members replay their step graphs
        # every member holds the runs tdoa_debug_owned_runs names, byte for byte
        for k in range(n_members):
            m = g.member(k)
            for s, n in enumerate(ns):
                runs = tdoa_amd.capi.owned_runs(n, min(ns), window_len, k, n_members)
                assert runs
                for first, count in runs:
                    assert np.array_equal(m.capture_download(s, first, count), raw[s][2 * first:2 * (first + count)])
    assert (want.shape[0] < n_members) == (window_len == BLOCK)
    assert got.tobytes() == want.tobytes()
    assert again.tobytes() == want.tobytes()


def test_group_over_captures_synthesised_on_each_member():
    """captures made on the members through tdoa_group_member (not by the group's ingest) are processed as well"""
    import tdoa_amd
    with tdoa_amd.Group([0, 0, 0], max_lag=MAX_LAG, window_len=WLEN) as g, \
            tdoa_amd.Context(max_lag=MAX_LAG, window_len=WLEN) as c:
        for target in [g.member(k) for k in range(3)] + [c]:
            for s in range(3):
                target.synth_capture(s, BLOCK, ST[s], TX, 0x5D0A0000 + s)
        want = c.process()
        assert g.process().tobytes() == want.tobytes()
    assert want.shape == (9, 3) and (want["abs_corr"] > 0).all()


def test_stacked_calls_of_different_sizes_share_the_merged_sum():
    """tdoa_group_process_stacked, _closure and _locate gather the members' fixed-point sums through one function and keep
    them in the group from call to call: stacks of 2, whole blocks, single windows and whole blocks again (9, 3, 15 and 3
    stacks of 6 pairs and 1399 lags) on one group of two members, each the single context's bytes.  Four stations, windows
    of 10 000, 5 per block: the geometry of the searches' four_stations fixtures."""
    import tdoa_amd
    wl, wpb, ml = 10_000, 5, 700
    table = np.random.default_rng(29).integers(-16 * 900, 16 * 900 + 1, size=(300, 4), dtype=np.int32)
    with tdoa_amd.Group([0, 0], max_lag=ml, window_len=wl) as g, tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        for target in [g.member(0), g.member(1), c]:
            for s in range(4):
                target.synth_capture(s, wpb * wl, ST[s % 3], TX, 0x5D0A0000 + s)
        g.locate_set_table(table, 20)        # (the group's binding sizes the map it returns from this call)
        c.locate_set_table(table, 20)
        calls = [("stacks of 2", lambda x: x.process_stacked(2, 3, 4, want_surface=True)),
                 ("closure, whole blocks", lambda x: {"closure": x.process_closure(0, 37, 2, (0, 13, -250, 100))}),
                 ("locate, single windows", lambda x: x.process_locate(1, 2, want_map=True)),
                 ("whole blocks", lambda x: x.process_stacked(0, 3, 4, want_surface=True))]
        for name, call in calls:
            got, want = call(g), call(c)
            assert sorted(got) == sorted(want), name
            for key in want:
                assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (name, key)
                assert got[key].tobytes() == want[key].tobytes(), (name, key)
        assert want["peaks"].shape == (3, 6, 3) and (want["peaks"]["abs_corr"][:, :, 0] > 0).all()


def test_members_with_different_stations_are_refused(tmp_path, oracle):
    import tdoa_amd
    paths = _write(tmp_path, oracle)
    with tdoa_amd.Group([0, 0], max_lag=MAX_LAG, window_len=WLEN) as g:
        g.capture_upload_files(paths)
        m = g.member(1)
        m.capture_clear()
        for s, p in enumerate(paths[:2]):    # member 1 now holds two stations, member 0 three
            m.capture_upload_file(s, p)
        out = np.zeros((9, 3), dtype=tdoa_amd.capi.PEAK_DTYPE)
        out["lag"] = 12345
        out["corr"] = -7.0
        before = out.tobytes()
        with pytest.raises(tdoa_amd.TdoaError) as e:
            g.process(out=out)
        assert e.value.status == 6 and "member 1 (device 0)" in str(e.value)     # TDOA_ERR_STATE
        assert out.tobytes() == before


def test_group_create_names_the_member_whose_device_does_not_exist():
    import tdoa_amd
    n = tdoa_amd.capi.load().tdoa_device_count()
    with pytest.raises(tdoa_amd.TdoaError) as e:
        tdoa_amd.Group([0, n])
    assert e.value.status == 2 and ("member 1 (device %d)" % n) in str(e.value)    # TDOA_ERR_NO_DEVICE


def test_group_over_two_devices_is_the_single_context(tmp_path, oracle):
    import tdoa_amd
    n = tdoa_amd.capi.load().tdoa_device_count()
    if n < 2:
        pytest.skip("tdoa_device_count() = %d: a group over devices [0, 1] needs two GPUs" % n)
    paths = _write(tmp_path, oracle)
    want = _single(paths, WLEN)
    with tdoa_amd.Group([0, 1], max_lag=MAX_LAG, window_len=WLEN) as g:
        g.capture_upload_files(paths)
        got = g.process()
    assert got.tobytes() == want.tobytes()
