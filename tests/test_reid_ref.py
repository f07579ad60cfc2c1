"""reid_ref, the plain-Python definition of re-identification, against xform_fpe_ref's de-identification of the
oracle's findings: the round trip over the corpus of test_gpu_fpe.py, the literal rows, and the output positions
against a recomputation that transforms every finding on its own and looks for it in the de-identified row."""
import pytest

import reid_ref as RR
import xform_configs as X
import xform_fpe_ref as FR
import xform_hash_ref
import xform_ref
from conftest import pkg

CONFIGS = {"F": FR.F, "FC": FR.FC}
# (input row, de-identified under F, re-identified)
LITERALS = [
    (b"card number 4111 1111 1111 1111 ok", b"card number 9329 9759 1240 5582 ok", None),
    (b"my ssn is 536-22-1234@johnny thanks", b"my ssn is 598-59-5178 thanks", b"my ssn is 536-22-1234 thanks"),
    (b"ip address 10.20.30.40 then card 4111 1111 1111 1111 ok",
     b"ip address [IP_ADDRESS] then card 9329 9759 1240 5582 ok",
     b"ip address [IP_ADDRESS] then card 4111 1111 1111 1111 ok"),
    (b"@bob_1 wrote from 10.20.30.40 call 212-555-0187 or mail jane.doe@corp.example.org",
     b" wrote from [IP_ADDRESS] call 287-927-8221 or mail c9eE.zSZ@61uc.bMX9S9N.0Xu",
     b" wrote from [IP_ADDRESS] call 212-555-0187 or mail jane.doe@corp.example.org"),
]


@pytest.fixture(scope="module")
def corpus(oracle_cfg):
    from oracle import pii_oracle as O
    synth = pkg("synth")
    bank = synth.build_bank(600, 600, seed=7)
    corp = synth.make_corpus(263, 37, bank, seed=3)
    rows = [(int(corp.conv_slot[i]), int(corp.role[i]),
             corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes(), int(corp.ts_us[i]))
            for i in range(corp.n)]
    return rows, O.process_rows(rows, oracle_cfg)


def _piece(row, f, names, cfg):
    """finding f of `row` transformed on its own"""
    return FR.apply_transform(row[f.start:f.end], [xform_hash_ref._Shift(f, f.start)], names, cfg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_round_trip_and_positions_over_the_corpus(name, corpus, oracle_cfg):
    rows, exp = corpus
    assert len(rows) == 9731
    cfg = X.with_block(CONFIGS[name])
    names = oracle_cfg.type_names
    decrypted = 0
    for r, x in zip(rows, exp):
        row, fs = r[2], x[1]
        de = FR.apply_transform(row, fs, names, cfg)
        # positions, independently: every finding transformed on its own, found in the de-identified row right
        # after the unchanged bytes that follow the previous one
        pos = RR.positions(fs, names, cfg)
        want, cur, prev_end, delta = [], 0, 0, 0
        for f, (lo, hi) in zip(fs, pos):
            tp = _piece(row, f, names, cfg)
            gap = row[prev_end:f.start]
            at = de.find(gap + tp, cur)
            assert at == cur and (lo, hi) == (at + len(gap), at + len(gap) + len(tp)) == (f.start + delta, lo + len(tp))
            is_fpe = FR.fpe_of(xform_ref.pick(names[f.type_id], cfg)) is not None
            want += [gap, row[f.start:f.end] if is_fpe else tp]
            decrypted += is_fpe
            cur, prev_end, delta = hi, f.end, delta + len(tp) - (f.end - f.start)
        want.append(row[prev_end:])
        assert de[cur:] == row[prev_end:]
        got = RR.reidentify(de, fs, names, cfg)
        assert got == b"".join(want), (row, de, got)
        if name == "FC":
            assert got == row
    if name == "FC":
        assert decrypted == sum(len(x[1]) for x in exp) == 1040
    else:
        assert decrypted > 0          # (no row of this corpus has an FPE finding behind a length change: the literals do)


def test_literals(oracle_cfg):
    from oracle import pii_oracle as O
    cfg = X.with_block(FR.F)
    names = oracle_cfg.type_names
    for row, de, back in LITERALS:
        fs = O.find_pii(row, oracle_cfg)
        assert FR.apply_transform(row, fs, names, cfg) == de
        assert RR.reidentify(de, fs, names, cfg) == (row if back is None else back)
    # row 3: a +1 delta before the card (11 input bytes at [11, 22), a 12-byte token); row 4: -6, then +1
    fs = O.find_pii(LITERALS[2][0], oracle_cfg)
    assert [(f.start, f.end) for f in fs] == [(11, 22), (33, 52)] and RR.positions(fs, names, cfg) == [(11, 23), (34, 53)]
    fs = O.find_pii(LITERALS[3][0], oracle_cfg)
    assert [names[f.type_id] for f in fs] == ["SOCIAL_HANDLE", "IP_ADDRESS", "PHONE_NUMBER", "EMAIL_ADDRESS"]
    assert [lo - f.start for f, (lo, _) in zip(fs, RR.positions(fs, names, cfg))] == [0, -6, -5, -5]


def test_out_of_range_bytes_stay(oracle_cfg):
    """a1b as PERSON_NAME under a NUMERIC catch-all: one numeral, below nmin = 2; its "***" stays "***" """
    cfg = X.with_block([{"primitive_transformation": FR.fpe_prim(FR.KA, "NUMERIC")}])
    names = oracle_cfg.type_names
    f = RR.Finding(2, 5, names.index("PERSON_NAME"))
    de = FR.apply_transform(b"x a1b y", [f], names, cfg)
    assert de == b"x *** y" and RR.reidentify(de, [f], names, cfg) == de
    assert RR.decrypt_piece(FR.KA, "0123456789", b"7") == b"7"
    assert RR.decrypt_piece(FR.KA, "0123456789", b"1" * 65) == b"1" * 65          # nmax = 64
    assert FR.limits(10) == (2, 64)
