"""GPU: okvfe::HipFrontend::propagationBlocks (and the host form HipFrontend::propagation) of the C++ host mirror,
through tests/cpp/imu_propagation_cli, equal the Python path okvfe_imu_propagation_blocks_device byte for byte, and both
equal the restatement."""
import os
import subprocess

import numpy as np
import pytest

import imu_scenes as SC
from okvis2_amd import capi

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "imu_propagation_cli")
FORMS = dict(mean=(False, False), jacobian=(True, False), covariance=(True, True))


def _python_path(fe, sc, form):
    jacobian, covariance = FORMS[form]
    n, n_cams = len(sc["mfs"]), len(sc["T_SC_params"])
    samples, begin, states = SC.pack(sc["mfs"])
    dev = [torch.from_numpy(a).cuda() for a in (samples, begin, states)]
    want = SC.expected([], n_cams)
    out = {k: torch.full((n,) + w.shape[1:], SC.SENTINEL, dtype=getattr(torch, str(w.dtype)), device="cuda")
           for k, w in want.items()}
    p = lambda k: out[k].data_ptr()
    res = capi.make_imu_result(p("pose"), p("speed_and_bias"), p("n_propagated"), p("status"), p("n_out_of_range"),
                               p("jacobian") if jacobian else None, p("covariance") if covariance else None, p("T_WC"),
                               p("gravity_C"))
    fe.imu_propagation_blocks_device(SC.PARAMS, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n,
                                     sc["T_SC_params"], res)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.parametrize("form", list(FORMS))
def test_cpp_mirror_equals_the_python_path(tmp_path, fp64_order, form):
    tree = fp64_order == "eigen_tree"
    jacobian, covariance = FORMS[form]
    sc = SC.scenes()[2]
    refs = SC.references(tree)[0][2]
    n, n_cams = len(sc["mfs"]), len(sc["T_SC_params"])
    fe = capi.Frontend(64, 64, 10.0, 0, 50, 10)
    try:
        py = _python_path(fe, sc, form)
    finally:
        fe.close()
    req = tmp_path / "req.bin"
    SC.write_request(req, sc["mfs"], sc["T_SC_params"], tree, jacobian, covariance)
    want = SC.expected(refs, n_cams, jacobian=jacobian, covariance=covariance)
    for mode in ((), ("host",)):
        resp = tmp_path / ("resp_" + "_".join(mode) + ".bin")
        r = subprocess.run([CLI, str(req), str(resp), *mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (mode, r.returncode, r.stdout, r.stderr)
        got = SC.read_response(resp, n, n_cams)
        for k, w in want.items():
            assert SC.same_bytes(got[k], py[k].reshape(got[k].shape)), (mode, form, k, "differs from the Python path")
            assert SC.same_bytes(got[k], w), (mode, form, k, "differs from the restatement")
