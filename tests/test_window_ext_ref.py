"""tests/window_ext_ref.py against the frozen oracle (no extras: the same function) and against known
answers written out by hand (the shipped rules)."""
from conftest import pkg

import window_ext_ref as WR


def _stream(n_conv, per_conv, seed):
    synth = pkg("synth")
    bank = synth.build_bank(400, 900, seed=seed)
    corp = synth.make_corpus(n_conv, per_conv, bank, seed=seed + 1)
    rows = []
    for i in range(corp.n):
        a, b = int(corp.offsets[i]), int(corp.offsets[i + 1])
        rows.append((int(corp.conv_slot[i]), int(corp.role[i]), corp.data[a:b].tobytes(), int(corp.ts_us[i])))
    return rows


def test_without_extras_the_helper_is_the_oracle(oracle_cfg):
    from oracle import pii_oracle as O
    rows = _stream(40, 12, seed=71)
    assert len(rows) == 40 * 12
    got = WR.process_window_rows_ext(rows, [[] for _ in rows], oracle_cfg, n=5)
    assert got == O.process_window_rows(rows, oracle_cfg, n=5)
    assert any(fs for _, fs, _ in got) and any(et for _, _, et in got)


def test_a_name_stays_with_its_row_until_the_row_leaves_the_window(oracle_cfg):
    from oracle import pii_oracle as O
    P = oracle_cfg.type_id["PERSON_NAME"]
    C = O.ROLE_CUSTOMER
    rows = [(7, C, b"my name is John Smith", 1)] + [(7, C, b"line %d" % k, 1 + k) for k in range(1, 7)]
    extras = [[(11, 21, P, 4)]] + [[] for _ in range(6)]
    out = WR.process_window_rows_ext(rows, extras, oracle_cfg, n=5)
    assert out[0][0] == b"my name is [PERSON_NAME]"
    assert out[1][0] == b"my name is [PERSON_NAME]\nline 1"
    assert out[4][0] == b"my name is [PERSON_NAME]\nline 1\nline 2\nline 3\nline 4"
    assert [(f.start, f.end, f.type_id, f.likelihood) for f in out[4][1]] == [(11, 21, P, 4)]
    assert out[5][0] == b"line 1\nline 2\nline 3\nline 4\nline 5"          # row 1 has left: so has its name
    assert out[5][1] == [] and out[6][1] == []


def test_candidates_are_shifted_and_resolved_against_rule_findings(oracle_cfg):
    from oracle import pii_oracle as O
    P = oracle_cfg.type_id["PERSON_NAME"]
    EM = oracle_cfg.type_id["EMAIL_ADDRESS"]
    C = O.ROLE_CUSTOMER
    t = b"I am John Smith, email jsmith@example.com thanks"
    assert len(t) == 48 and t[23:41] == b"jsmith@example.com"
    # second row of its window (offset 6): a candidate that loses to the longer email at its start, one
    # starting inside the kept email, one below min_likelihood (POSSIBLE), one that stands alone
    rows = [(3, C, b"hello", 1), (3, C, t, 2)]
    out = WR.process_window_rows_ext(rows, [[], [(5, 15, P, 4), (23, 29, P, 5), (30, 35, P, 5), (42, 48, P, 2)]],
                                     oracle_cfg)
    assert out[1][0] == b"hello\nI am [PERSON_NAME], email [EMAIL_ADDRESS] thanks"
    assert [(f.start, f.end, f.type_id) for f in out[1][1]] == [(11, 21, P), (29, 47, EM)]
    # ... and one that wins: longer than the email at the same start
    out = WR.process_window_rows_ext(rows, [[], [(23, 48, P, 4)]], oracle_cfg)
    assert out[1][0] == b"hello\nI am John Smith, email [PERSON_NAME]"
    assert [(f.start, f.end, f.type_id, f.likelihood) for f in out[1][1]] == [(29, 54, P, 4)]
    # below min_likelihood alone: nothing
    out = WR.process_window_rows_ext(rows[:1], [[(0, 5, P, 2)]], oracle_cfg)
    assert out[0][0] == b"hello" and out[0][1] == []


def test_join_extras_offsets():
    text, joined = WR.join_extras([(b"ab", [(0, 2, 9, 4)]), (b"", []), (b"cde", [(1, 3, 9, 5)])])
    assert text == b"ab\n\ncde"
    assert joined == [(0, 2, 9, 4), (5, 7, 9, 5)]
