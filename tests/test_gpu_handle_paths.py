"""The handle kernels against what the library computed while a vertex list and a face list ran through kernels of their own (the recordings
tests/golden/handle_paths_*.npz of tests/golden/gen_handle_paths.py, which lists the cases and the quantities).  Both kinds of list now go through
the corner-list kernels of csrc/k_handle.hpp:
  a face list keeps its kernels' expressions word for word -- every recorded quantity has the recorded bits, the positions after three time steps
  on the factorised path included;
  a vertex list is held to 1e-14 of the largest entry of each quantity, the bar tests/test_gpu_surface_handles.py sets for a face list of corner
  points against the vertex list, and the verdict "same bits: yes / no" is printed per quantity.  Measured on an MI355X: yes for all thirteen.  (The
  one-lane-per-handle kernels compiled F += k w (x - t) and vals += k w to one fused multiply-add each; the NC = 1 branches of k_handle_grad and
  k_handle_hess keep that expression per entry.  Summing the entries from zero first, as NC = 3 does, moved matrix entries by one unit in the last
  place, 1.7e-16 of the largest entry.)"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_handle_paths as gen  # noqa: E402

pytestmark = pytest.mark.gpu


def _pair(name):
    want = dict(np.load(os.path.join(HERE, "golden", "handle_paths_%s.npz" % name)))
    got = gen.record(name)
    assert set(got) == set(want)
    return got, want


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_a_face_list_keeps_its_bits(name):
    got, want = _pair(name)
    assert want["pos_after_3_steps"].shape == (169, 3) and want["frame_wrench"].shape == ((3, 6) if name == "dense" else (0, 6))
    same = {k: np.array_equal(got[k], want[k]) for k in sorted(want)}
    print("same bits: " + ", ".join("%s %s" % (k, "yes" if v else "no") for k, v in same.items()))
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert same[k], (k, float(np.abs(got[k] - want[k]).max()))


def test_a_vertex_list_stays_within_1e_14_of_the_largest_entry():
    got, want = _pair("vertex")
    assert want["handle_points"].shape == (270, 3) and want["frame_wrench"].shape == (3, 6) and "pos_after_3_steps" not in want
    rel = {}
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        rel[k] = float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max())
        print("%-14s max difference %.2e of the largest entry, same bits: %s" % (k, rel[k], "yes" if np.array_equal(got[k], want[k]) else "no"))
    for k in sorted(want):
        assert rel[k] <= 1e-14, (k, rel[k])
