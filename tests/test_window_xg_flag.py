"""PII_WINDOW_XG through the Python layers, without a GPU: the constant equals the header's and shares no bit
with the other two flags, the engine's window_enable takes incremental_exclusions last, and the service passes
it on only when asked (by default its call is window_enable(window_n, slot_bytes))."""
import inspect
import os
import re

from conftest import ROOT, pkg
from test_service_window_ext import _WindowExtEngine, _row
from test_service import Clock


def test_constant_equals_the_header():
    with open(os.path.join(ROOT, "include", "pii_engine.h")) as f:
        m = re.search(r"^#define\s+PII_WINDOW_XG\s+(\d+)", f.read(), re.M)
    assert m, "include/pii_engine.h defines PII_WINDOW_XG"
    E = pkg("engine")
    assert E.PII_WINDOW_XG == int(m.group(1)) == 16
    assert E.PII_WINDOW_XG & (E.PII_WINDOW_FULL | E.PII_WINDOW_XF) == 0


def test_window_enable_has_the_keyword():
    p = inspect.signature(pkg("engine").Engine.window_enable).parameters
    assert list(p)[-1] == "incremental_exclusions" and p["incremental_exclusions"].default is False
    assert list(p)[:5] == ["self", "window_n", "slot_bytes", "full", "incremental_transforms"]
    q = inspect.signature(pkg("service").PiiService.rescan_window_batch).parameters
    assert list(q)[-1] == "incremental_exclusions" and q["incremental_exclusions"].default is False


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
    svc.rescan_window_batch([_row("a", "again", 11)], incremental_exclusions=True)     # already enabled
    assert len(eng.enabled) == 1
    eng = _Recording(oracle_cfg)
    svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload")
    svc.rescan_window_batch([_row("a", "hello", 10)], window_n=4, slot_bytes=4096, incremental_exclusions=True)
    assert eng.enabled == [((4, 4096), {"incremental_exclusions": True})]
    eng = _Recording(oracle_cfg)
    svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload")
    svc.rescan_window_batch([_row("a", "hello", 10)], incremental_transforms=True, incremental_exclusions=True)
    assert eng.enabled == [((5, 8192), {"incremental_transforms": True, "incremental_exclusions": True})]
