"""GPU: the ONE-STREAM schedule of the scale space (capi_detect.cpp: detect_layers_staged).  A scale-space call runs its
layers side by side on streams of their own unless stage profiling (or heavy-kernel chaining) is on; then the same
per-layer steps are issued grouped by stage on the caller's stream, so that a stage timer brackets a whole stage.  The
configurations are those of tests/test_gpu_octaves.py (Harris score, octaves 1 and 3) and tests/test_gpu_agast.py
(OKVFE_SCORE_BRISK_SCALESPACE): keypoints, descriptors and counts with profiling on are byte-equal to those with
profiling off, both equal the oracle, and the profile holds one launch bracket per stage per call."""
import numpy as np
import pytest

import gpu_common as G
from okvis2_amd import capi, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STAGES = ("harris", "nms", "sort", "select", "describe", "compact")


def _harris_case(w, h, octaves, seed):
    B = 3
    imgs = np.stack([synth.corners_image(w, h, seed + 10 * i) for i in range(B)])
    make = lambda: capi.Frontend(w, h, 30.0, octaves, 100, 300, max_batch=B, max_candidates=0)
    ref = lambda oracle, img: oracle.detect_describe(img, 30.0, octaves, 100, 300, oracle.MODE_GRADIENT)
    return imgs, make, ref


def _brisk_case(octaves, maxk):
    w, h = 752, 480
    imgs = np.stack([synth.corners_image(w, h, 5), synth.noise_image(w, h, 6)])
    make = lambda: capi.Frontend(w, h, 0.0, octaves, 34, maxk, rotation_invariant=False, max_batch=len(imgs),
                                 score_type=capi.SCORE_BRISK_SCALESPACE, max_candidates=1 << 16)
    ref = lambda oracle, img: oracle.detect_describe(img, 0.0, octaves, 34, maxk, oracle.MODE_UPRIGHT, None, None,
                                                     np.float32(1.0), (0.0, 1.0, 0.0),
                                                     score_type=oracle.SCORE_BRISK_SCALESPACE)
    return imgs, make, ref


CASES = {
    "harris-octaves1": lambda: _harris_case(752, 480, 1, 5),
    "harris-octaves3": lambda: _harris_case(1024, 1024, 3, 7),
    "brisk-scalespace-octaves2": lambda: _brisk_case(2, 450),
}


def _run(fe, d_img, B, stream):
    fe.detect_describe_batch_device(d_img.data_ptr(), B, None, None, stream)
    stream.synchronize()
    fe.check_capacity(B)
    return [fe.download(i) for i in range(B)]


def _assert_same(a, b):
    assert len(a) == len(b)
    for (ka, da, _, _), (kb, db, _, _) in zip(a, b):
        assert len(ka) == len(kb)  # counts
        assert ka.tobytes() == kb.tobytes() and da.tobytes() == db.tobytes()


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_stream_scale_space_equals_side_by_side_and_the_oracle(oracle, case):
    imgs, make, ref = CASES[case]()
    B = len(imgs)
    want = [ref(oracle, imgs[i]) for i in range(B)]
    d_img = torch.from_numpy(imgs).cuda()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    fe = make()
    plain = _run(fe, d_img, B, st)          # layers side by side
    fe.profile_enable(True)
    calls = 2
    staged = [_run(fe, d_img, B, st) for _ in range(calls)]   # one stream, grouped by stage
    p = fe.profile_read()
    fe.profile_enable(False)
    again = _run(fe, d_img, B, st)          # ... and side by side again on the same context
    for i in range(B):
        G.assert_keypoints_equal(plain[i][0], want[i][0])
        assert np.array_equal(plain[i][1], want[i][1])
        assert len(want[i][0]) > 50
    for got in staged + [again]:
        _assert_same(got, plain)
    assert {k: p[k][1] for k in STAGES} == {k: calls for k in STAGES}, p
    assert p["harris"][0] > 0.0 and p["describe"][0] > 0.0, p
    assert len({int(o) for i in range(B) for o in np.unique(want[i][0]["octave"])}) >= 2
    # a context that never ran the side-by-side schedule gives the same
    fresh = make()
    fresh.profile_enable(True)
    _assert_same(_run(fresh, d_img, B, st), plain)
