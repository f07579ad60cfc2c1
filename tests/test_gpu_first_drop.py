"""Absorbed match starts on the GPU: first_begin drops a start that finditer always skips before its
FIRST run (compiler.add_first_drop).  Final outputs must not change: bit-exact parity vs the oracle on
rows built around the rule's edge cases, on 128-byte lanes (a small batch), with the drop on, with
it off (PII_FIRST_DROP=0) and with a blob that lacks the det.first_pre section; and one window
re-scan (N = 5) vs process_window_rows.
"""
import os

import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

COUNTEREXAMPLE = b"@-@11.aa-.@1-.bZ1.%._1"
LONG_LOCAL = b"first.middle.last_with-a.very.long.local%part+tag"      # > 16 bytes: continuation path


def _engine(blob, env):
    E = pkg("engine")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return E.Engine(blob, device=0, n_conv_slots=4096)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=["drop", "switch_off", "old_blob"])
def eng(compiled, request):
    comp = pkg("compiler")
    blob = compiled.blob
    if request.param == "old_blob":             # a blob compiled before the section existed
        S = comp.blob_sections(blob)
        del S["det.first_pre"]
        blob = comp._sections_to_blob(S)
    e = _engine(blob, {"PII_FIRST_DROP": "0"} if request.param == "switch_off" else {})
    yield e
    e.close()


def _rows():
    """a few hundred short rows and some ~400-byte rows (cut into 128-byte lanes)"""
    synth = pkg("synth")
    bank = synth.build_bank(60, 120, seed=41)
    texts = [
        COUNTEREXAMPLE,
        b"x " + COUNTEREXAMPLE + b" y",
        b"a@b.co1x@y.org",
        b"mail a@b.co1x@y.org now",
        LONG_LOCAL + b"@example.com",
        b"write to " + LONG_LOCAL + b"@mail.example.org please",
        # an address at row start after a row that ends in a byte of X: its first start is kept
        b"my address follows abc.def",
        b"jane.doe@example.com is the address",
        b"ends with percent%",
        b"j@x.io",
        # SOCIAL_HANDLE next to an address: the exclusion rule still sees the accepted email match
        b"jane.doe@example.com @TechieTom",
        b"ping @TechieTom or tom.techie@example.com, thanks",
        b"tom@techie.example.com@TechieTom",
        b"a.b@c.de1f.g@h.ij2k@l.mn",
        b"x@y.org" * 9,
        b"....@....a@b.cc....",
        b"%%%%a@b.ccc%%%%d@e.ff",
    ]
    # ~400-byte rows: addresses straddling the lane cuts wherever they fall (every 128 bytes of the
    # batch), by sliding the addresses through the row
    words = b"please note that the shipment will arrive on monday morning before noon at the usual place "
    for shift in range(0, 128, 5):
        row = bytearray()
        row += words[:shift % len(words)]
        while len(row) < 400:
            row += b"so " + LONG_LOCAL[:7 + shift % 23] + b"@example.com, " + words[:30 + shift % 17]
        texts.append(bytes(row))
    texts += list(bank.texts[:180])
    return texts


def _spans(res, i):
    m = res.spans["utt"] == i
    return [(int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans[m]]


@pytest.fixture(scope="module")
def expected(oracle_cfg):
    from oracle import pii_oracle as O
    texts = _rows()
    rows = [(i // 8, O.ROLE_CUSTOMER, t, 1_000_000 + i) for i, t in enumerate(texts)]
    return rows, O.process_rows(rows, oracle_cfg)


def test_parity_vs_oracle(eng, expected):
    rows, exp = expected
    assert 200 <= len(rows) <= 400
    res = eng.scan_redact([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [r for _, r, _, _ in rows],
                          [s for _, _, _, s in rows])
    assert eng.stats()["lane_bytes"] == 128
    for i, (red, fs, _, _) in enumerate(exp):
        assert res.text(i) == red, (i, rows[i][2], res.text(i), red)
        assert _spans(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, rows[i][2])
    # the counterexample's second match starts where the first ended (an absorbed position)
    assert [(s, e) for s, e, _, _ in _spans(res, 0)] == [(1, 8), (8, 16)]


def test_window_rescan(compiled, oracle_cfg):
    from oracle import pii_oracle as O
    C, A = O.ROLE_CUSTOMER, O.ROLE_AGENT
    e = _engine(compiled.blob, {})
    try:
        e.window_enable(5, 8192, full=False)
        assert e.window_mode() == "incremental"
        rows = [(7, A, b"what is your email address?", 1),
                (7, C, b"it is jane.doe@example.com and also abc.def", 2),      # ends with bytes of X
                (7, C, b"ghi@mail.example.org is my other one", 3),              # starts with bytes of X
                (7, C, COUNTEREXAMPLE, 4),
                (7, C, b"a@b.co1x@y.org", 5),
                (7, C, LONG_LOCAL + b"@example.com @TechieTom", 6),
                (7, C, b"x1%", 7),
                (7, C, b"y2@z.org", 8),
                (8, C, b"tom.techie@example.com", 1),
                (8, C, b"@TechieTom tom@example.com", 2)]
        store, hist = O.ContextStore(), {}
        groups = list(oracle_cfg.context_keywords.keys())
        for call in (rows[:3], rows[3:6], rows[6:]):
            res = e.rescan_window([t for _, _, t, _ in call], [c for c, _, _, _ in call], [r for _, r, _, _ in call],
                                  [s for _, _, _, s in call])
            exp = O.process_window_rows(call, oracle_cfg, n=5, store=store, history=hist)
            for i, ((red, fs, et), row) in enumerate(zip(exp, call)):
                assert res.text(i) == red, (i, row, res.text(i), red)
                assert _spans(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, row)
                g = int(res.ctx_info[i])
                assert (groups[g] if g >= 0 else None) == et, (i, row)
    finally:
        e.close()
