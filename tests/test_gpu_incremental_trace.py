"""The call traces of tests/test_incremental_trace.py on the device route (LZS_ROUTE=device: every call a launch -- the
pinned box, the staged copies, the many-wavefront pass with the size it learns), against the `device` section of
tests/golden/inc_call_traces.json, recorded on the MI355X from a build of the commit before lzs_incremental.c was
restructured.  A record without that section is a failure, not a skip."""
import pytest

import test_incremental_trace as T

torch = pytest.importorskip("torch")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(T.SCENARIOS))
def test_every_call_on_the_device_route_does_what_was_recorded(monkeypatch, name):
    assert torch.cuda.is_available(), "the device route needs a GPU (it has no fallback)"
    monkeypatch.setenv("LZS_ROUTE", "device")
    T.replay("device", name)
