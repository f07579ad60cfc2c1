"""The case lists of validator_cases reach what they claim to reach: conditions on the inputs, checked under the
oracle alone (no GPU).  test_gpu_validators.py runs the same lists on the device."""
import os

import pytest
import yaml

import validator_cases as VC
from conftest import pkg


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """rule file name -> (oracle RuleConfig, compiled rules), loaded from files as a user's would be"""
    from oracle import pii_oracle as O
    comp = pkg("compiler")
    with open(os.path.join(comp.RULES_DIR, "builtin_infotypes.yaml")) as f:
        shipped = yaml.safe_load(f)
    d = tmp_path_factory.mktemp("validators")
    out = {}
    for name, make in (("short", VC.builtin_short), ("long", VC.builtin_long)):
        cfg, builtin = VC.write_rules(d, name, make(shipped))
        out[name] = (O.RuleConfig.load(cfg, builtin), comp.compile_default(cfg, builtin))
    return out


@pytest.fixture(scope="module")
def cases():
    """(rule file, validator) -> [(label, row, accepted under the oracle's validator)]"""
    from oracle import pii_oracle as O
    out = {}
    for name, gens in (("short", VC.SHORT_CASES), ("long", VC.LONG_CASES)):
        for kind, gen in gens.items():
            out[name, kind] = [(label, row, O.VALIDATORS[kind](VC.value_of(row))) for label, row in gen()]
    return out


def _detectors(ocfg, types):
    return [d for d in ocfg.detectors if d.type_name in types]


def test_the_rule_files_compile_and_hold_what_they_should(rules):
    short, long_ = rules["short"][0], rules["long"][0]
    assert {d.validator for d in short.detectors} == set(VC.KINDS)
    assert len(short.detectors) == 9                          # the nine shipped detectors with a validator
    assert {d.type_name: d.validator for d in long_.detectors} == {
        n: d["validator"] for n, d in VC.LONG_DETECTORS.items()}
    for ocfg, comp in rules.values():
        assert all(d.likelihood == 4 for d in ocfg.detectors)
        assert comp.blob[:8] == b"PIIRULE1"
        assert not ocfg.variant(None).rule_sets


def test_labels_are_unique_and_rows_are_small(cases):
    labels = [label for rows in cases.values() for label, _, _ in rows]
    assert len(labels) == len(set(labels))
    assert 10000 < len(labels) < 60000
    assert max(len(row) for rows in cases.values() for _, row, _ in rows) < 128


def test_every_value_is_its_detectors_match_and_findings_follow_the_validator(rules, cases):
    """the detector's regex matches exactly the value, so a rejected case is rejected by the validator and not
    by a typo; under the short rule file the finding is there exactly when the validator accepts"""
    from oracle import pii_oracle as O
    for (name, kind), rows in cases.items():
        ocfg = rules[name][0]
        types = (VC.SHORT_TYPES if name == "short" else VC.LONG_TYPES)[kind]
        dets = _detectors(ocfg, types)
        assert dets and all(d.validator == kind for d in dets)
        ids = {ocfg.type_id[t] for t in types}
        for label, row, ok in rows:
            span = (2, len(row) - 2)
            assert any(m.span() == span for d in dets for m in d.regex.finditer(row)), label
            found = [f for f in O.find_pii(row, ocfg) if (f.start, f.end) == span and f.type_id in ids]
            assert bool(found) == ok, label
            if name == "short" and not ok:
                assert not O.find_pii(row, ocfg), label


def test_every_width_class_has_an_accepted_and_a_rejected_case(cases):
    seen = {}
    for (name, kind), rows in cases.items():
        for _, row, ok in rows:
            seen.setdefault((kind, VC.width_class(len(row) - 4)), set()).add(ok)
    want = {k: ["16", "32", "33+"] for k in ("luhn", "nanp", "ssn", "ein", "ipv4", "iban")}
    want["swift"] = ["16"]                                    # 8 or 11 bytes: all the pattern produces
    assert sorted(seen) == sorted((k, w) for k, ws in want.items() for w in ws)
    for key, oks in seen.items():
        assert False in oks, key
        assert (True in oks) == (key not in VC.NEVER_ACCEPTED), key


def test_the_tables_are_covered_entry_by_entry(cases):
    from oracle import pii_oracle as O
    for form in ("8", "11"):
        rows = [(label, ok) for label, _, ok in cases["short", "swift"]
                if label.startswith("swift/%s/" % form) and "/edge/" not in label]
        assert len(rows) == 676
        assert {label[-2:] for label, ok in rows if ok} == set(O.ISO3166)
        assert sum(ok for _, ok in rows) == len(O.ISO3166) == 249
    edges = [(label, ok) for label, _, ok in cases["short", "swift"] if "/edge/" in label]
    assert all(ok == ("/DE/" in label) for label, ok in edges) and len(edges) == 2 * (2 * 8 + 2 * 14)
    for key, per in ((("short", "ein"), 1), (("long", "ein"), 4)):
        rows = cases[key]
        assert len(rows) == 100 * per
        assert sum(ok for _, _, ok in rows) == len(O.EIN_PREFIXES) * per
        assert {int(label[-2:]) for label, _, ok in rows if ok} == set(O.EIN_PREFIXES)
    for key in (("short", "nanp"), ("long", "nanp")):
        for label, _, ok in cases[key]:
            assert ok == (label[-2] >= "2" and label[-1] >= "2"), label
    assert len(cases["short", "nanp"]) == 500 and len(cases["long", "nanp"]) == 400
    assert len(cases["short", "ssn"]) == 72 and len(cases["long", "ssn"]) == 288
    assert sum(ok for _, _, ok in cases["short", "ssn"]) == 4 * 2 * 2       # areas 001 665 667 899


def test_every_luhn_group_of_ten_accepts_exactly_one(cases):
    for key in (("short", "luhn"), ("long", "luhn")):
        groups = {}
        for label, row, ok in cases[key]:
            groups.setdefault(label.rsplit("/", 1)[0], []).append(ok)
        assert len(groups) == 2 * (len(VC.LUHN_FORMS) if key[0] == "short" else 2 * len(VC.LUHN_LONG_COUNTS))
        for g, oks in groups.items():
            assert len(oks) == 10 and sum(oks) == 1, g
    counts = {sum(c in b"0123456789" for c in VC.value_of(row)) for _, row, _ in cases["short", "luhn"]}
    assert counts == set(range(13, 20))


def test_iban_lengths_checks_and_the_intermediate_reduction(cases):
    by_len = {}
    tops = []
    for label, row, ok in cases["short", "iban"]:
        v = VC.value_of(row)
        length = len(v.replace(b" ", b""))
        by_len.setdefault((length, b" " in v), set()).add(ok)
        tops.append(VC.iban_running_max(v))
        if b" " in v:
            assert len(v) == length + (length - 1) // 4
    assert sorted(by_len) == [(n, s) for n in VC.IBAN_LENGTHS for s in (False, True)]
    for (length, _), oks in by_len.items():
        assert oks == ({True, False} if 15 <= length <= 34 else {False}), length
    spaced = {len(VC.value_of(row)) for label, row, _ in cases["short", "iban"] if "/spaced/" in label}
    assert {36, 37, 38, 39, 41, 42, 43} <= spaced and min(spaced) == 14    # 29 .. 35 characters: MemSrc
    # the running value reaches 1 << 24 (several times in one value: a 'Z' run grows it by 100 per character),
    # and without the intermediate reduction it would pass 1 << 32
    assert sum(t >= 1 << 24 for t in tops) > len(tops) // 2
    zrun = VC.iban_values()[-1][1].encode()
    assert zrun[4:] == b"Z" * 31
    tail, reductions = 0, 0
    for c in zrun[4:]:
        tail = tail * 100 + c - 55
        if tail >= 1 << 24:
            tail, reductions = tail % 97, reductions + 1
    assert reductions >= 8
    # letters and digits in the head: every country's letters at 0 and 1, every digit at 2 and 3
    heads = {VC.value_of(row)[:4] for _, row, _ in cases["short", "iban"] if b" " not in VC.value_of(row)}
    assert {h[:2].decode() for h in heads} == set(VC.IBAN_COUNTRIES)
    assert {h[2:].decode() for h in heads} == set(VC.IBAN_CHECKS)


def test_ipv4_boundaries_and_shapes(cases):
    from oracle import pii_oracle as O
    for pos in range(4):
        got = {label.rsplit("/", 1)[1]: ok for label, _, ok in cases["short", "ipv4"]
               if label.startswith("ipv4/field%d/" % pos)}
        assert got == {v: int(v) <= 255 for v in VC.IPV4_FIELDS}
    long_ = {label: ok for label, _, ok in cases["long", "ipv4"]}
    assert [s for s in VC.IPV4_SHAPES if long_["ipv4_long/shape/" + s]] == [
        "1.2.3.4", "255.255.255.255", "0.0.0.0", "000.000.000.000"]
    assert not any(ok for label, ok in long_.items() if "/wide" in label or "/mid4" in label)
    assert O.v_ipv4(b"1.2.3.255") and not O.v_ipv4(b"1.2.3.256")


def test_alignment_families(rules):
    """accepted and rejected as named; the siblings differ where they say; over the sixteen start offsets the
    matches end 16, 17, 32, 33, 47 and 48 bytes past their first 16-byte boundary"""
    from oracle import pii_oracle as O
    ends = {}
    for name, rule_file, kind, acc, sibs in VC.alignment_families():
        V = O.VALIDATORS[kind]
        assert V(acc.encode()), name
        ocfg = rules[rule_file][0]
        for which, s in sibs.items():
            assert not V(s.encode()) and len(s) == len(acc), (name, which)
            diff = [i for i in range(len(acc)) if acc[i] != s[i]]
            assert diff == [{"last": len(acc) - 1, "first": 0, "b4": 4, "b5": 5}[which]], (name, which)
        for v in [acc] + list(sibs.values()):
            at = [(f.start, f.end) for f in O.find_pii(VC.embed(v.encode()), ocfg)]
            assert ((2, 2 + len(v)) in at) == (v == acc), (name, v)
            if rule_file == "short":                  # (under the long rules another detector may match a part)
                assert at == ([(2, 2 + len(v))] if v == acc else []), (name, v)
        for off in range(16):
            row = VC.place(acc.encode(), off)
            assert len(row) % 16 == 0 and row[off:off + len(acc)] == acc.encode()
            assert VC.place(acc.encode(), off, last=True).endswith(acc.encode())
            ends.setdefault(kind, set()).add((off + len(acc), len(acc) > 32))
    for kind in ("luhn", "iban"):
        assert {(e, False) for e in (16, 17, 32, 33, 47)} <= ends[kind]        # RegSrc: one, two, three chunks
        assert {(e, True) for e in (33, 47, 48, 49)} <= ends[kind]             # MemSrc
    for kind in ("nanp", "ssn", "ein"):
        assert {(e, False) for e in (16, 17, 32, 33)} <= ends[kind], kind
        assert {(e, True) for e in (47, 48)} <= ends[kind], kind
    assert {(e, False) for e in (16, 17)} <= ends["swift"] & ends["ipv4"]
