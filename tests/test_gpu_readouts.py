"""The energy, the read-outs of system identification (elastic_force, param_grad, friction_grad, param_grads) and the reverse step, replayed bit
for bit against tests/golden/readouts_{drape,balancing}.npz: what the library computed before these kernels and entry points moved into
csrc/k_scene.hpp, k_adjoint.hpp, adjoint_api.hpp and param_api.hpp (tests/golden/gen_readouts.py records and replays the cases)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_readouts  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", gen_readouts.CASES)
def test_readouts_and_reverse_steps_keep_their_bits(name):
    want = np.load(os.path.join(HERE, "golden", "readouts_%s.npz" % name))
    # the fixture reaches what it is there for: live contacts and body keys on `balancing`, non-trivial cloth keys and reverse steps on both
    assert np.count_nonzero(want["keys_all"]) >= 3 and np.count_nonzero(want["keys_all_1"]) >= 3
    assert np.abs(want["pos_grad"][0]).max() > 0 and np.abs(want["angleref_grad"][0]).max() > 0
    if name == "balancing":
        assert want["contact_counts"][0] > 0 and np.abs(want["elastic_force"]).max() > 0 and np.abs(want["tmp_z_frozen_1"]).max() > 0
    got = gen_readouts.record(name)
    assert sorted(got) == sorted(want.files)
    differ = [k for k in sorted(got) if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    assert not differ, differ
