"""Host side of the post-processing entry points: argument validation without a launch, and the host-side MSSEG
detection test against the reference's results (tests/golden/postprocessing.npz)."""
import ctypes

import numpy as np
import pytest
import torch

from segmentation_pipeline_amd import _lib
from segmentation_pipeline_amd import evaluators as E
from segmentation_pipeline_amd import post_processing as PP

FAKE = ctypes.c_void_p(256)   # never dereferenced: every call below fails its checks before a launch


def test_ccl_rejects_bad_volumes_and_connectivity():
    L = _lib.lib()
    assert L.m355_ccl_workspace(8, 8, 8) > 8 ** 3 * 4
    assert L.m355_ccl_workspace(0, 8, 8) == 0
    rc = L.m355_ccl_label(FAKE, FAKE, FAKE, 0, 4, 4, 1, 0, FAKE, 1 << 20, None)
    assert rc == -1 and b"ccl_label" in L.m355_last_error()
    rc = L.m355_ccl_label(FAKE, FAKE, FAKE, 1 << 11, 1 << 10, 1 << 10, 1, 0, FAKE, 1 << 20, None)
    assert rc == -1 and b"2^31" in L.m355_last_error()
    for conn in (0, 4, -1):
        rc = L.m355_ccl_label(FAKE, FAKE, FAKE, 4, 4, 4, conn, 0, FAKE, 1 << 20, None)
        assert rc == -1 and b"connectivity" in L.m355_last_error()
    rc = L.m355_ccl_label(FAKE, FAKE, FAKE, 4, 4, 4, 1, 2, FAKE, 1 << 20, None)
    assert rc == -1 and b"mode" in L.m355_last_error()
    rc = L.m355_ccl_label(FAKE, FAKE, FAKE, 64, 64, 64, 3, 0, FAKE, 16, None)
    assert rc == -4 and b"workspace" in L.m355_last_error()


def test_dilation_histogram_and_casts_reject_bad_arguments():
    L = _lib.lib()
    rc = L.m355_masked_dilate6(FAKE, FAKE, 4, 4, 4, FAKE, FAKE, None, None, 0, FAKE, None)
    assert rc == -1 and b"src == dst" in L.m355_last_error()
    rc = L.m355_masked_dilate6(FAKE, ctypes.c_void_p(512), 4, -4, 4, FAKE, FAKE, None, None, 0, FAKE, None)
    assert rc == -1 and b"masked_dilate6" in L.m355_last_error()
    rc = L.m355_masked_dilate6(FAKE, ctypes.c_void_p(512), 4, 4, 4, FAKE, FAKE, FAKE, None, 0, FAKE, None)
    assert rc == -1 and b"rank_class" in L.m355_last_error()
    rc = L.m355_label_histogram(FAKE, None, 64, 0, 0, 0, FAKE, None, None)
    assert rc == -1 and b"bins" in L.m355_last_error()
    rc = L.m355_label_histogram(FAKE, None, 1 << 31, 0, 0, 4, FAKE, None, None)
    assert rc == -1 and b"label_histogram" in L.m355_last_error()
    rc = L.m355_label_histogram(FAKE, FAKE, 64, 0, 0, 4, FAKE, None, None)
    assert rc == -1 and b"bstride" in L.m355_last_error()
    rc = L.m355_label_convert_in(FAKE, 7, 0, FAKE, 64, FAKE, None)
    assert rc == -1 and b"dtype" in L.m355_last_error()
    rc = L.m355_label_convert_out(None, None, None, FAKE, 3, 64, None)
    assert rc == -1 and b"label_convert_out" in L.m355_last_error()


def test_python_layer_rejects_bad_input_before_the_device():
    with pytest.raises(ValueError):
        PP.label(np.zeros((2, 2, 2), np.int32), connectivity=4)
    with pytest.raises(TypeError):
        PP.remove_holes([[[0]]], 64)


@pytest.mark.parametrize("tag", ["pair0", "pair1", "pair2_empty_pred"])
def test_msseg_detection_test_matches_reference(golden, tag):
    g = golden("postprocessing.npz")
    h = torch.from_numpy(g[f"{tag}/hist"])
    got_t = E.msseg_detection_test(h)
    got_p = E.msseg_detection_test(h.T)
    assert got_t.tolist() == g[f"{tag}/det_target"].tolist()
    assert got_p.tolist() == g[f"{tag}/det_pred"].tolist()
    # an int64 table, as overlap_histogram returns it, gives the same verdicts (float32 arithmetic on the host)
    assert E.msseg_detection_test(h.to(torch.int64)).tolist() == got_t.tolist()


def test_detection_test_parameters():
    # one target (10 voxels), two predictions covering 6 and 2 of them; prediction 1 also spills 30 voxels
    h = torch.tensor([[0, 30, 0], [2, 6, 2], ], dtype=torch.float32)
    assert E.msseg_detection_test(h).tolist() == [False]                      # precision 6/36 < 0.3
    assert E.msseg_detection_test(h, min_precision=0.1).tolist() == [True]   # 6/8 of the overlap >= 0.65
    assert E.msseg_detection_test(h, min_recall=0.9).tolist() == [False]     # recall 0.8


def test_num_is_taken_as_a_python_int():
    # keep_components(img, img.max()): a numpy or 0-d tensor scalar of the map's dtype becomes a Python int
    assert PP._as_int(np.uint8(3), "num") == 3 and type(PP._as_int(np.uint8(3), "num")) is int
    assert PP._as_int(torch.tensor(200, dtype=torch.uint8), "num") == 200
    assert PP._as_int(np.int64(-2), "num") == -2 and PP._as_int(4.0, "num") == 4
    assert 2 - 1 - PP._as_int(np.uint8(3), "num") == -2
    for bad in (2.5, True, "3"):
        with pytest.raises(TypeError):
            PP._as_int(bad, "num")
