"""The workspace sizes of the three tiled heads (egv_egonce_long_work_floats, egv_egonce_queue_work_floats, egv_sigmoid_head_work_floats)
and egv_egonce_queue_layout against the layout arithmetic restated in tests/egonce_long_ref.py / tests/egonce_queue_ref.py, which was
written down when the long and the queue head each had a layout function of their own: the shared one must give both their numbers
exactly -- a caller's workspace and the queue buffers are sized by them.  Host code: no device is needed."""
import ctypes
import itertools
import os

import pytest

import egonce_long_ref as R
import egonce_queue_ref as QR

NS = (1, 63, 64, 65, 1024, 1025, 4100, 65536)
DS = (4, 64, 68, 256)
VOCAB = ((0, 0), (582, 118))
QS = (64, 128, 2048, 65536)


@pytest.fixture(scope="module")
def h():
    from egovlp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libegovlp_hip.so not built (run __graft_entry__.build())")
    return _lib.lib()


def test_long_and_sigmoid_work_floats(h):
    for n, D, (dn, dv) in itertools.product(NS, DS, VOCAB):
        assert h.egv_egonce_long_work_floats(n, D, dn, dv) == R.long_work_floats(n, D, dn, dv) > 0, (n, D, dn, dv)
        assert h.egv_sigmoid_head_work_floats(n, D, dn, dv) == R.sigmoid_work_floats(n, D, dn, dv) > 0, (n, D, dn, dv)


def test_queue_work_floats(h):
    for n, D, (dn, dv), Q in itertools.product(NS, DS, VOCAB, QS):
        want = QR.queue_work_floats(n, D, dn, dv, Q)
        assert (want > 0) == (n <= Q)
        assert h.egv_egonce_queue_work_floats(n, D, dn, dv, Q) == want, (n, D, dn, dv, Q)


def test_the_rectangular_split_of_a_square_is_the_square_split():
    """what lets one layout function serve both heads: without queue tiles the queue head's split is the long head's"""
    for n, D, (dn, dv) in itertools.product(NS, DS, VOCAB):
        L = R.prep_layout(n, D, dn, dv)
        assert QR.rect_split(L["ntiles"], L["ntiles"], R.STAT_WGS) == R.split(L["ntiles"], R.STAT_WGS)
        assert QR.rect_split(L["ntiles"], L["ntiles"], R.GRAD_WGS) == R.split(L["ntiles"], R.GRAD_WGS)


def test_refused_sizes_return_zero(h):
    for n, D, dn, dv in [(0, 256, 582, 118), (-1, 256, 0, 0), (65537, 256, 582, 118), (64, 2, 0, 0), (64, 6, 0, 0), (64, 260, 0, 0),
                         (64, 256, -1, 0), (64, 256, 0, -1), (64, 256, 65537, 0), (64, 256, 0, 65537)]:
        assert R.long_work_floats(n, D, dn, dv) == 0 and R.sigmoid_work_floats(n, D, dn, dv) == 0
        assert h.egv_egonce_long_work_floats(n, D, dn, dv) == 0, (n, D, dn, dv)
        assert h.egv_sigmoid_head_work_floats(n, D, dn, dv) == 0, (n, D, dn, dv)
        assert h.egv_egonce_queue_work_floats(n, D, dn, dv, 65536) == 0, (n, D, dn, dv)
    for n, Q in [(64, 0), (64, 32), (64, 100), (64, 65600), (64, -64), (65, 64), (129, 128)]:
        assert QR.queue_work_floats(n, 256, 582, 118, Q) == 0
        assert h.egv_egonce_queue_work_floats(n, 256, 582, 118, Q) == 0, (n, Q)


def test_queue_layout(h):
    Dp, W = ctypes.c_int32(), ctypes.c_int32()
    for D, (dn, dv) in itertools.product(DS + (6, 260, 0), VOCAB + ((1, 1), (128, 129), (-1, 0), (0, 65537))):
        want = QR.queue_layout(D, dn, dv)
        rc = h.egv_egonce_queue_layout(D, dn, dv, ctypes.byref(Dp), ctypes.byref(W))
        assert (rc == 0) == (want is not None), (D, dn, dv)
        if want is not None:
            assert (Dp.value, W.value) == want, (D, dn, dv)
    assert h.egv_egonce_queue_layout(256, 582, 118, None, ctypes.byref(W)) == 1
    assert h.egv_egonce_queue_layout(256, 582, 118, ctypes.byref(Dp), None) == 1
