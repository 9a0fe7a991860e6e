"""GPU: the routes of the searches on the stacks' sums return the same bytes (csrc/stack_search.inc).

Every search is reached (a) by a context's own call, whose kernels are nodes of the step graph, (b) by its *_from_q entry on
the caller's words, and (c) by the group's call on the members' merged sum.  The three drivers are written once; the seven
entries are the closure search, the clock search, the clock-line search and the four of the delay-table family.

What the other files assert already, per entry: (a) = (c), a group of two members on one device against a single context, in
test_group_returns_a_single_contexts_bytes of test_gpu_closure.py, test_gpu_sync.py, test_gpu_sync_drift.py, test_gpu_locate.py,
test_gpu_locate_multi.py, test_gpu_locate_track.py and test_gpu_locate_track_multi.py.  None of them compares (a) with (b):
the own call and the *_from_q entry meet only through the numpy models, each on words of its own.  That equality is what
this file adds: every output of the own call against the *_from_q entry fed the partial_host of tdoa_process_stacked on the
same captures.

The smallest shapes that run the drivers: 3 stations (one triple; closure once more on 4 stations, four triples), max_lag 64,
four windows per block in stacks of two -- two stacks per block, so tracks and lines have two positions, and every stack is
full, as the one n_w of a *_from_q call wants -- and a table of 8 x 8 cells.  Byte equality: no tolerance."""
import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes
from test_locate_cpu import ST4

pytestmark = pytest.mark.gpu

ML, WL, WPB, M = 64, 2048, 4, 2
TX = (41.20, -96.00, 400.0)
REF = np.array([0, 16, 40, 72], dtype=np.int32)
CENTRE = np.array([0, 1, -2, 1], dtype=np.int32)

# entry -> (own call, the same on the caller's words); c: the context, S: stations, Q: the stacks' sums
ENTRIES = {
    "closure": (lambda c, S: c.process_closure(M, 4, 2, CENTRE[:S]),
                lambda c, S, Q: c.closure_from_q(Q, S, M, 4, 2, CENTRE[:S])),
    "sync": (lambda c, S: c.process_sync(REF[:S], M, 4, 2, CENTRE[:S]),
             lambda c, S, Q: c.sync_from_q(Q, REF[:S], M, 4, 2, CENTRE[:S])),
    "sync_drift": (lambda c, S: c.process_sync_drift(REF[:S], M, 4, 2, 3, 2, CENTRE[:S]),
                   lambda c, S, Q: c.sync_drift_from_q(Q, REF[:S], WPB // M, M, 4, 2, 3, 2, CENTRE[:S])),
    "locate": (lambda c, S: c.process_locate(M, 2, want_map=True),
               lambda c, S, Q: c.locate_from_q(Q, S, M, 2)),
    "locate_multi": (lambda c, S: c.process_locate_multi(M, 2, 1, 2, want_map=True),
                     lambda c, S, Q: c.locate_multi_from_q(Q, S, M, 2, 1, 2)),
    "locate_track": (lambda c, S: c.process_locate_track(M, 1, 2, want_total=True),
                     lambda c, S, Q: c.locate_track_from_q(Q, S, WPB // M, M, 1, 2)),
    "locate_track_multi": (lambda c, S: c.process_locate_track_multi(M, 1, 2, 1, 2, want_total=True),
                           lambda c, S, Q: c.locate_track_multi_from_q(Q, S, WPB // M, M, 1, 2, 1, 2)),
}


@pytest.fixture(scope="module")
def captured():
    """S -> (context with S stations' captures and an 8 x 8 table, the sums Q of its stacks of two windows), made on demand"""
    import tdoa_amd
    made = {}

    def get(S):
        if S not in made:
            c = tdoa_amd.Context(max_lag=ML, window_len=WL)
            for s in range(S):
                c.synth_capture(s, WPB * WL, ST4[s], TX, 0x57AC0000 + s)
            assert c.num_windows()[0] == WPB and c.num_stacks(M) == (WPB // M, 3 * WPB // M)
            c.locate_set_table(np.random.default_rng(19).integers(0, 16 * 30, size=(64, S), dtype=np.int32), 8)
            Q = c.process_stacked(M, 1, 1, want_partial=True)["partial"]
            assert Q.shape == (3 * WPB // M, S * (S - 1) // 2, 2 * ML - 1) and Q.any()
            made[S] = (c, Q)
        return made[S]

    yield get
    for c, _ in made.values():
        c.close()


@pytest.mark.parametrize("entry,S", [(name, 3) for name in ENTRIES] + [("closure", 4)])
def test_own_call_and_from_q_return_the_same_bytes(captured, entry, S):
    c, Q = captured(S)
    own, from_q = ENTRIES[entry]
    a, b = own(c, S), from_q(c, S, Q)
    if not isinstance(a, dict):
        a, b = {"records": a}, {"records": b}
    assert a.keys() == b.keys()
    assert any(v.tobytes().strip(b"\0") for v in a.values())         # (something was found: the outputs are not all zero)
    assert all(_same_bytes(a[k], b[k]) for k in a), [k for k in a if not _same_bytes(a[k], b[k])]
    again = own(c, S)                                                # the own call replays its graph after the debug call's uploads
    again = again if isinstance(again, dict) else {"records": again}
    assert all(_same_bytes(again[k], a[k]) for k in a)
