"""More patterns live in one row than the finditer tracker has register slots (FinditerTracker, LIVE):
the (pattern, end) list it moves to, on the batch path (k_select / k_sel_fix) and on the incremental
window path (k_win_cands), against the oracle.  Needs an MI355X: pytest -m gpu.

Rule set: the shipped config plus seven digit-run types, [0-9]{21} .. [0-9]{27}.  At the first byte of
a run of 60 digits every one of them has a finditer match, so the sixth finds no free slot."""
import os

import pytest

import excl_configs as XC
from conftest import pkg
from test_gpu_parity import _check_rows
from test_gpu_window import _check as _check_window

pytestmark = pytest.mark.gpu

LIVE = 5                                 # pii_device.h
RUNS = [("RUN%d" % k, "[0-9]{%d}" % k) for k in range(21, 28)]

ROW60 = b"ref " + b"9" * 60 + b" ok"
ROWS = [b"hello, how can I help you today",
        ROW60,
        b"ref " + b"9" * 60 + b" and " + b"8" * 60 + b" ok",     # the list is looked up again after it was built
        b"id " + b"7" * 700 + b" end",                           # cut over several 128-byte lanes
        b"thanks, that is all"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(compiled rules, the oracle's view of them), once the oracle alone has shown the property the
    tests rely on: at the first byte of every run, more than LIVE detectors have a finditer match"""
    from oracle import pii_oracle as O
    path = XC.write(tmp_path_factory.mktemp("live"), "runs", XC.with_custom([], custom=RUNS))
    ocfg = O.RuleConfig.load(path)
    enabled = ocfg.variant(None).enabled_types
    for text, first in ((ROWS[1], 4), (ROWS[2], 4), (ROWS[2], 69), (ROWS[3], 3)):
        assert text[first - 1:first] == b" " and text[first:first + 1].isdigit()
        live = sum(1 for det in ocfg.detectors if det.type_name in enabled and
                   any(m.start() == first for m in det.regex.finditer(text)))
        assert live >= LIVE + 1, (text[:20], first, live)
    assert O.redact(ROW60, ocfg, None)[0] == b"ref [RUN27][RUN27]999999 ok"
    return pkg("compiler").compile_default(path), ocfg


def _rows(conv):
    from oracle import pii_oracle as O
    return [(conv, O.ROLE_CUSTOMER, t, 1000 * (i + 1)) for i, t in enumerate(ROWS)]


def test_batch_path(runs):
    E = pkg("engine")
    eng = E.Engine(runs[0].blob, device=0, n_conv_slots=64)
    try:
        _check_rows(eng, runs[1], _rows(3))
    finally:
        eng.close()


@pytest.mark.parametrize("env", [{}, {"PII_WIN_LONG": "1"}], ids=["whole_rows", "cut_rows"])
def test_window_path(runs, env):
    """the conversation's rows over two calls: the ring holds rows whose candidates came through the list;
    cut_rows: k_win_cands walks the 700-digit row across its lanes, every one of which holds candidates (only
    the thread of the lane the row starts in may walk them)"""
    E = pkg("engine")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = E.Engine(runs[0].blob, device=0, n_conv_slots=64)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        eng.window_enable(5, 8192)
        assert eng.window_mode() == "incremental"
        rows = _rows(9)
        _check_window(eng, runs[1], [rows[:3], rows[3:]])
    finally:
        eng.close()
