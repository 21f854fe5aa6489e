"""GPU: the drop-in symbols of the correction monomials (tmlqcd_hip_{ratcor, cloverratcor, ndratcor, ndcloverratcor}_{heatbath, acc})
called from a host stub on host fields, in both residency modes, against the reference's fixtures (tests/golden/ref_ratcor_*).  One
fresh child process per mode (tests/ratcor_dropin_child.py), as the other *_dropin_child.py.  Bounds: tests/ratcor_restate.py::gpu_bound."""
import json
import os

import pytest

from tests import ratcor_restate as rr
from tests.hostprog import run_child

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_dropin_symbols(mode):
    errs = run_child("ratcor_dropin_child.py", mode)
    print(errs)
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_ratcor_scalars_4x4.json")))
    assert errs["sw_invert_failures"] == 0.0 and errs["sw_invert_nd_failures"] == 0.0
    assert errs["g_mu_moved"] == 0.0
    for name in rr.TYPES:
        t = s["types"][name]
        for k in ("heatbath_iters", "heatbath_napp", "acc_iters", "acc_napp"):
            assert errs["%s_%s" % (name, k)] == 0, (name, k)
        for k in ("energy0", "energy1", "pf"):
            assert errs["%s_%s" % (name, k)] <= rr.gpu_bound(t, k), (name, k, errs["%s_%s" % (name, k)])
