"""The dispatch-order feedback (python-ray-tracer_amd/csrc/rt_feedback.h behind dispatch() and launch_one()) on the GPU: the call
sequences of tests/algo/feedback_trace_cases.py must make, step by step, the decisions tests/golden/feedback_trace.npz records from
the library as it was before the rules became a header of their own."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, load_frame

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(REPO, "tests", "algo"))
try:
    import feedback_trace_cases as ftc
finally:
    sys.path.pop(0)


@pytest.mark.parametrize("remeasure", ftc.REMEASURES)
@pytest.mark.parametrize("name", sorted(ftc.SCRIPTS))
def test_feedback_trace_is_the_recorded_one(name, remeasure):
    """Script A (launches of every variant on three streams, camera and scene changes, rt_stream_forget, twelve geometries over
    the eight slots, a one-block frame) and Script B (static rt_render_sequence calls of 5 frames, 4 per launch, on fresh and on
    settled geometries: the unsettled-sequence path) on a context created under MI355RT_REMEASURE, the launching stream
    synchronised after every step.  The deltas of launches, frames, launches_measuring, launches_settled and table_builds of every
    step equal the recorded ones, and the last launch leaves the fixture's frame."""
    want = np.load(os.path.join(REPO, "tests", "golden", "feedback_trace.npz"))
    assert tuple(want["fields"]) == ftc.FIELDS
    rows, frame = ftc.replay(ftc.SCRIPTS[name], remeasure)
    ref = want[f"{name}/{remeasure}"]
    assert rows.shape == ref.shape
    bad = np.flatnonzero((rows != ref).any(axis=1))
    assert bad.size == 0, [(int(j), ftc.SCRIPTS[name][j], rows[j].tolist(), ref[j].tolist()) for j in bad[:5]]
    assert np.array_equal(frame, load_frame(ftc.FIXTURE)["frame_u8"])
