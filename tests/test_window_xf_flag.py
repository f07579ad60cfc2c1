"""PII_WINDOW_XF through the Python layers, without a GPU: the constant equals the header's, the engine's
window_enable takes incremental_transforms, and the service passes it on only when asked (by default its
call is window_enable(window_n, slot_bytes), which is all the other tests' engine doubles accept)."""
import inspect
import os
import re

from conftest import ROOT, pkg
from test_service_window_ext import _WindowExtEngine, _row
from test_service import Clock


def test_constant_equals_the_header():
    with open(os.path.join(ROOT, "include", "pii_engine.h")) as f:
        m = re.search(r"^#define\s+PII_WINDOW_XF\s+(\d+)", f.read(), re.M)
    assert m, "include/pii_engine.h defines PII_WINDOW_XF"
    E = pkg("engine")
    assert E.PII_WINDOW_XF == int(m.group(1)) == 2
    assert E.PII_WINDOW_XF & E.PII_WINDOW_FULL == 0


def test_window_enable_has_the_keyword():
    p = inspect.signature(pkg("engine").Engine.window_enable).parameters
    assert "incremental_transforms" in p and p["incremental_transforms"].default is False
    assert list(p)[:4] == ["self", "window_n", "slot_bytes", "full"]


class _Recording(_WindowExtEngine):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.enabled = []

    def window_enable(self, *a, **kw):
        self.enabled.append((a, kw))
        self.window_n = a[0]


def test_service_passes_the_keyword_only_on_request(oracle_cfg):
    S = pkg("service")
    eng = _Recording(oracle_cfg)
    svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload")
    svc.rescan_window_batch([_row("a", "hello", 10)])
    assert eng.enabled == [((5, 8192), {})]
    svc.rescan_window_batch([_row("a", "again", 11)], incremental_transforms=True)     # already enabled
    assert len(eng.enabled) == 1
    eng = _Recording(oracle_cfg)
    svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload")
    svc.rescan_window_batch([_row("a", "hello", 10)], window_n=4, slot_bytes=4096, incremental_transforms=True)
    assert eng.enabled == [((4, 4096), {"incremental_transforms": True})]
