"""The validators on the GPU (csrc/pii_device.h validate(): v_digits, v_luhn ... v_iban, through RegSrc / load32
for matches of at most 32 bytes and MemSrc for longer ones) against oracle.VALIDATORS, on the case lists of
validator_cases: the two lookup tables entry by entry, every boundary of the range checks, every start
alignment and chunk count, both call sites (the batch path's pair evaluation, the window path's).

Every row of every list is compared with O.process_rows on the same rows -- spans (utt, start, end, info_type,
likelihood), output bytes, offsets and the histogram; none is sampled or skipped.  Rule files (validator_cases):
"short" = the shipped patterns of the validated detectors alone, where a rejected value gives no finding at all;
"long" = detectors whose matches exceed 32 bytes; "shipped" = the shipped rules, where a rejected card number
may still be an account number and the oracle decides.  test_validator_cases.py (no GPU) checks that the lists
reach what they claim to.  Needs an MI355X: pytest -m gpu."""
import os

import numpy as np
import pytest
import yaml

import validator_cases as VC
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rules(tmp_path_factory, oracle_cfg, compiled):
    """rule file name -> (oracle RuleConfig, compiled rules)"""
    from oracle import pii_oracle as O
    comp = pkg("compiler")
    with open(os.path.join(comp.RULES_DIR, "builtin_infotypes.yaml")) as f:
        shipped = yaml.safe_load(f)
    d = tmp_path_factory.mktemp("validators")
    out = {"shipped": (oracle_cfg, compiled)}
    for name, make in (("short", VC.builtin_short), ("long", VC.builtin_long)):
        cfg, builtin = VC.write_rules(d, name, make(shipped))
        out[name] = (O.RuleConfig.load(cfg, builtin), comp.compile_default(cfg, builtin))
    return out


@pytest.fixture(scope="module")
def engines(rules):
    E = pkg("engine")
    made = {}

    def get(name):
        if name not in made:
            made[name] = E.Engine(rules[name][1].blob, device=0, n_conv_slots=1 << 12)
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _rows(texts, role=2):
    # role OTHER: no context is kept or used; a conversation's rows are contiguous, sixteen to a slot
    assert len(texts) <= 16 << 12
    return [(i // 16, role, t, 0) for i, t in enumerate(texts)]


def _spans_of(exp):
    return [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]


def _check_host(eng, texts, ocfg, labels=None):
    """host entry point: every row's bytes, the offsets, the spans and the histogram"""
    from oracle import pii_oracle as O
    rows = _rows(texts)
    exp = O.process_rows(rows, ocfg)
    eng.histogram_reset()
    res = eng.scan_redact(texts, [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows])
    for i, x in enumerate(exp):
        assert res.text(i) == x[0], (labels[i] if labels else i, texts[i], res.text(i), x[0])
    assert [int(o) for o in res.out_offsets] == [0] + list(np.cumsum([len(x[0]) for x in exp]))
    got = [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"]))
           for s in res.spans]
    assert got == _spans_of(exp)
    hist = eng.histogram()
    assert (hist == np.bincount(res.spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    return exp


def _check_device(eng, texts, ocfg, labels):
    """device entry point, the text buffer at a 16-byte-aligned base and not a byte longer than the rows: the
    same comparison; returns the rows' start offsets in the buffer"""
    import torch
    from oracle import pii_oracle as O
    E = pkg("engine")
    dev = torch.device("cuda:0")
    data, offs = E.pack(texts)
    n = len(texts)
    exp = O.process_rows(_rows(texts), ocfg)
    out_cap = sum(len(x[0]) for x in exp) + 64
    span_cap = sum(len(x[1]) for x in exp) + 64
    d_text = torch.from_numpy(data.copy()).to(dev)
    assert d_text.data_ptr() % 16 == 0 and d_text.numel() == int(offs[n])
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(dev)
    d_slot = torch.from_numpy((np.arange(n, dtype=np.uint32) // 16).view(np.int32)).to(dev)
    d_role = torch.full((n,), 2, dtype=torch.uint8, device=dev)
    d_ts = torch.zeros(n, dtype=torch.int64, device=dev)
    d_out = torch.full((out_cap,), 0xEE, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.empty(n, dtype=torch.int16, device=dev)
    eng.histogram_reset()
    eng.scan_redact_device(d_text.data_ptr(), d_offs.data_ptr(), n, d_slot.data_ptr(), d_role.data_ptr(),
                           d_ts.data_ptr(), d_out.data_ptr(), out_cap, d_oo.data_ptr(), d_sp.data_ptr(), span_cap,
                           d_ctx.data_ptr())
    ob, ns, flags = eng.sync()
    assert flags == 0
    out, oo = d_out.cpu().numpy()[:ob].tobytes(), d_oo.cpu().numpy()
    spans = np.frombuffer(d_sp[:ns * 16].cpu().numpy().tobytes(), dtype=E.SPAN_DTYPE)
    for i, x in enumerate(exp):
        assert out[int(oo[i]):int(oo[i + 1])] == x[0], (labels[i], texts[i])
    assert [int(o) for o in oo] == [0] + list(np.cumsum([len(x[0]) for x in exp]))
    got = [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in spans]
    assert got == _spans_of(exp)
    hist = eng.histogram()
    assert (hist == np.bincount(spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    return exp, offs


def _count(exp, ocfg, types):
    ids = {ocfg.type_id[t] for t in types}
    return sum(f.type_id in ids for x in exp for f in x[1])


# ------------------------------------------------------------------- 1 exhaustive tables and boundaries
@pytest.mark.parametrize("kind", VC.KINDS)
def test_short_forms_under_the_reduced_rules(kind, rules, engines):
    """a rejected value gives no finding at all: the span list is the validator's verdict"""
    from oracle import pii_oracle as O
    ocfg = rules["short"][0]
    cases = VC.SHORT_CASES[kind]()
    exp = _check_host(engines("short"), [r for _, r in cases], ocfg, [label for label, _ in cases])
    for (label, row), x in zip(cases, exp):
        assert bool(x[1]) == O.VALIDATORS[kind](VC.value_of(row)), label


@pytest.mark.parametrize("kind", VC.KINDS)
def test_short_forms_under_the_shipped_rules(kind, rules, engines):
    cases = VC.SHORT_CASES[kind]()
    _check_host(engines("shipped"), [r for _, r in cases], rules["shipped"][0], [label for label, _ in cases])


@pytest.mark.parametrize("kind", list(VC.LONG_CASES))
def test_long_forms(kind, rules, engines):
    from oracle import pii_oracle as O
    ocfg = rules["long"][0]
    cases = VC.LONG_CASES[kind]()
    exp = _check_host(engines("long"), [r for _, r in cases], ocfg, [label for label, _ in cases])
    tid = ocfg.type_id[VC.LONG_TYPES[kind][0]]
    for (label, row), x in zip(cases, exp):
        own = [f for f in x[1] if f.type_id == tid and (f.start, f.end) == (2, len(row) - 2)]
        assert bool(own) == O.VALIDATORS[kind](VC.value_of(row)), label


# --------------------------------------------------------------------------------- 2 mixed wavefront
def _interleaved(gens, per_kind):
    """row k of kind k % len(gens), each kind's cases cycled: neighbouring pairs hold different validators"""
    lists = [gen() for gen in gens.values()]
    steps = [next(p for p in (37, 41, 43, 47) if len(cases) % p) for cases in lists]    # coprime to the length
    out = []
    for i in range(per_kind):
        for cases, step in zip(lists, steps):
            out.append(cases[(i * step) % len(cases)])
    return out


@pytest.mark.parametrize("name", ["short", "long"])
def test_mixed_wavefront(name, rules, engines):
    gens = VC.SHORT_CASES if name == "short" else VC.LONG_CASES
    cases = _interleaved(gens, 512)
    ocfg = rules[name][0]
    exp = _check_host(engines(name), [r for _, r in cases], ocfg, [label for label, _ in cases])
    types = VC.SHORT_TYPES if name == "short" else VC.LONG_TYPES
    for kind in gens:
        n = _count(exp, ocfg, types[kind])
        assert 0 < n < 512, kind                            # every kind is accepted and rejected in the mix


def test_one_row_with_a_value_of_every_kind(rules, engines):
    from oracle import pii_oracle as O
    fams = {}
    for name, rule_file, kind, acc, sibs in VC.alignment_families():
        fams.setdefault((rule_file, kind), (acc, list(sibs.values())))
    for rule_file in ("short", "long"):
        vals = [v for (rf, _), v in fams.items() if rf == rule_file]
        good = b"x " + b" | ".join(acc.encode() for acc, _ in vals) + b" y"
        bad = b"x " + b" | ".join(s[0].encode() for _, s in vals if s) + b" y"
        ocfg = rules[rule_file][0]
        exp = _check_host(engines(rule_file), [good, bad, good + b" " + bad], ocfg)
        assert len(exp[0][1]) == len(vals) and len(O.find_pii(bad, ocfg)) < len(vals)


# ------------------------------------------------------------- 3 every alignment, every chunk count
@pytest.mark.parametrize("rule_file", ["short", "long"])
def test_every_start_alignment_and_the_end_of_the_buffer(rule_file, rules, engines):
    """each family's accepted value and its siblings at the sixteen start offsets of a 16-byte-aligned buffer
    (every row is a multiple of 16 bytes), so a match of n bytes at offset off takes one, two or three aligned
    chunks in load32 and crosses MemSrc's windows at every phase; then each once as the last bytes of the buffer"""
    ocfg, eng = rules[rule_file][0], engines(rule_file)
    fams = [f for f in VC.alignment_families() if f[1] == rule_file]
    texts, labels, where = [], [], []
    for name, _, kind, acc, sibs in fams:
        for which, v in [("acc", acc)] + sorted(sibs.items()):
            for off in range(16):
                texts.append(VC.place(v.encode(), off))
                labels.append("%s/%s/off%d" % (name, which, off))
                where.append((off, len(v), which == "acc"))
    exp, offs = _check_device(eng, texts, ocfg, labels)
    for i, (off, n, ok) in enumerate(where):
        assert (int(offs[i]) + off) % 16 == off
        at = [(f.start, f.end) for f in exp[i][1]]
        assert ((off, off + n) in at) == ok, labels[i]
        if rule_file == "short":
            assert at == ([(off, off + n)] if ok else []), labels[i]
    # the match ending at offsets[n]: one batch per value, the value's row last
    head = texts[:3]
    for name, _, kind, acc, sibs in fams:
        for which, v in [("acc", acc)] + sorted(sibs.items()):
            off = (len(name) + len(which)) % 16
            last = VC.place(v.encode(), off, last=True)
            exp, offs = _check_device(eng, head + [last], ocfg, ["head"] * 3 + ["%s/%s/last" % (name, which)])
            assert int(offs[4]) == int(offs[3]) + off + len(v)
            assert ((off, off + len(v)) in [(f.start, f.end) for f in exp[3][1]]) == (which == "acc"), (name, which)


# --------------------------------------------------------------------------------- 4 window call site
def _window_rows(rule_file):
    """conversations of seven rows (the window holds five): each family's accepted value and a sibling, short
    and padded past one 128-byte scan lane, interleaved with plain rows"""
    fams = [f for f in VC.alignment_families() if f[1] == rule_file]
    rows = []
    for c, (name, _, kind, acc, sibs) in enumerate(fams):
        rej = sorted(sibs.items())[0][1] if sibs else acc[:-1]
        pad = (VC.FILL * 2)[:118 - (c % 16)] + b" "
        texts = [VC.embed(acc.encode()), b"thanks", VC.embed(rej.encode()), pad + acc.encode() + b" ok",
                 b"", pad + rej.encode(), acc.encode() + b" " + rej.encode()]
        rows.append([(c + 1, k & 1, t, 10 + k) for k, t in enumerate(texts)])
    return rows


@pytest.mark.parametrize("rule_file", ["short", "long"])
def test_window_rescan_whole_cut_and_full(rule_file, rules):
    """the validators from the window path's pair evaluation: rows whole, rows cut at every scan lane
    (PII_WIN_LONG=1, read when the engine is created) and the full re-scan give the oracle's windows.
    (Regression: most rows of batches 4 and 6 are of 129 .. 256 bytes; cut at one lane they overflowed the
    long-row list, sized for rows of more than two lanes, and the call failed with PII_E_DEVICE.)"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    ocfg, comp = rules[rule_file]
    convs = _window_rows(rule_file)
    made = []
    try:
        for mode, env in (("incremental", {}), ("incremental", {"PII_WIN_LONG": "1"}), ("full", {})):
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                eng = E.Engine(comp.blob, device=0, n_conv_slots=256)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            made.append(eng)
            eng.window_enable(5, 8192, full=mode == "full")
            assert eng.window_mode() == mode
        store, hist = O.ContextStore(), {}
        found = 0
        for k in range(7):
            batch = [conv[k] for conv in convs]
            args = ([r[2] for r in batch], [r[0] for r in batch], [r[1] for r in batch], [r[3] for r in batch])
            got = [eng.rescan_window(*args) for eng in made]
            exp = O.process_window_rows(batch, ocfg, n=5, store=store, history=hist)
            for i, (red, fs, _) in enumerate(exp):
                for res in got:
                    assert res.text(i) == red, (k, i, batch[i])
                    m = res.spans["utt"] == i
                    assert [(int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"]))
                            for s in res.spans[m]] == [(f.start, f.end, f.type_id, f.likelihood) for f in fs]
                assert got[0].text(i) == got[1].text(i) == got[2].text(i)      # incremental = cut = full re-scan
                found += len(fs)
        assert found > 5 * len(convs)
    finally:
        for eng in made:
            eng.close()


# ---------------------------------------------------------------------------- 5 bytes around the match
# Every byte value 1 .. 255 but "\n" directly before and directly after an accepted value.  The row contract
# (include/pii_engine.h, pii_scan_redact: "row i = bytes[offsets[i] .. offsets[i+1])") forbids no byte value, so
# none is left out beyond the two this test was given without: 0 and "\n", the window path's join.  Bytes of
# 0x80 and above are non-word, as in Python's bytes re.
AROUND = {"luhn": "luhn_bare16", "nanp": "nanp_dash", "ssn": "ssn", "ein": "ein", "ipv4": "ipv4_12",
          "swift": "swift8", "iban": "iban22"}


@pytest.mark.parametrize("kind", VC.KINDS)
def test_every_byte_before_and_after_an_accepted_value(kind, rules, engines):
    acc = next(f[3] for f in VC.alignment_families() if f[0] == AROUND[kind]).encode()
    texts, labels = [], []
    for b in range(1, 256):
        if b == 10:
            continue
        texts += [b"x " + bytes([b]) + acc + b" y", b"x " + acc + bytes([b]) + b" y"]
        labels += ["%s/before/%02x" % (kind, b), "%s/after/%02x" % (kind, b)]
    assert len(texts) == 2 * 254
    ocfg = rules["short"][0]
    exp = _check_host(engines("short"), texts, ocfg, labels)
    whole = sum(any((f.end - f.start) == len(acc) for f in x[1]) for x in exp)
    assert 2 * 128 <= whole < 2 * 254                       # every byte of 0x80 and above leaves the match whole
