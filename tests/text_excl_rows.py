"""Rows for the text exclusion tests (configs: text_excl_configs), with known answers written by hand.
No GPU here: `python tests/text_excl_rows.py` prints what the reference makes of them and the counts of
rows the rules decide."""
from conftest import pkg

# (row, redacted under text_excl_configs.hand(), no context) -- literal, not computed
HAND = [
    # regex FULL_MATCH (default); \b at the quote's edges holds although the row has none there
    (b"orders ORD-01234 and ORD-51234", b"orders ORD-01234 and [ORDER_ID]"),
    (b"xORD-01234x ORD-012345678", b"xORD-01234x ORD-012345678"),
    # regex PARTIAL_MATCH
    (b"see ORD-9912 or ORD-1299", b"see ORD-9912 or [ORDER_ID]"),
    # dictionary FULL (case folded), PARTIAL (a word of the quote), INVERSE
    (b"a Red car, a dark RED door, a green one", b"a Red car, a dark RED door, a [COLOR] one"),
    (b"teal or blue", b"teal or [COLOR]"),
    # exclude_by_hotword, window_before: inside the window, outside it, the window clipped at the row start
    (b"a sample TK12345 vs TK54321 here", b"a sample TK12345 vs [TICKET] here"),
    (b"sample TK11111", b"sample TK11111"),
    (b"samples TK11111", b"samples [TICKET]"),
    # exclude_by_hotword, window_after: \A at the window start, \Z at its end and at the clipped row end
    (b"BG1234void ok", b"BG1234void ok"),
    (b"BG1234 avoid it", b"[BADGE] avoid it"),
    (b"BG1234 void", b"BG1234 void"),
    (b"BG1234 a void b", b"[BADGE] a void b"),
    # a dropped candidate still excludes another (PARTIAL exclude_info_types): the ZIP5 inside the dropped ZIP9
    (b"zip z00000-1234 ok", b"zip z00000-1234 ok"),
    (b"zip z12345-1234 ok", b"zip [ZIP9] ok"),
    # a dropped long candidate frees a shorter overlapping one of another type
    (b"REF TST 123456", b"REF [SHORTREF]"),
    (b"REF ABC 123456", b"[LONGREF]"),
    # a dropped match whose pattern's next start lies inside it: finditer has moved past "zbb"
    (b"xzbb zbb", b"xzbb [RUN]"),
    # one-byte quotes
    (b"# % #", b"# [MARK] #"),
    # INVERSE on a built-in type
    (b"call 800-555-0187 or 212-555-0187", b"call [PHONE_NUMBER] or 212-555-0187"),
]

# rows under text_excl_configs.context_cfg(): (row, context type or None, redacted)
CONTEXT = [
    (b"ip 10.1.2.3 and 11.1.2.3", None, b"ip 10.1.2.3 and 11.1.2.3"),              # IP_ADDRESS is not enabled
    (b"ip 10.1.2.3 and 11.1.2.3", "IP_ADDRESS", b"ip 10.1.2.3 and [IP_ADDRESS]"),  # ... but under its context
    (b"fax 212-555-0187", None, b"fax 212-555-0187"),                                # the same in every variant
    (b"fax 212-555-0187", "IP_ADDRESS", b"fax 212-555-0187"),
    (b"tel 212-555-0187", "PHONE_NUMBER", b"tel [PHONE_NUMBER]"),
]


def random_rows(group_types, n=4000, seed=31):
    """n synth customer rows under no context and under every context group: rows (slot, role, text, ts), slot
    0 none and slot 1 + g the context group g, and the context each slot must hold before the call"""
    from oracle import pii_oracle as O
    bank = pkg("synth").build_bank(0, n, seed=seed).texts
    rows, contexts = [], {}
    for slot in range(1 + len(group_types)):
        if slot:
            contexts[slot] = slot - 1
        rows += [(slot, O.ROLE_CUSTOMER, t, 1000) for t in bank]
    return rows, contexts


def oracle_store(contexts, group_types):
    from oracle import pii_oracle as O
    store = O.ContextStore()
    for slot, g in contexts.items():
        store.set(slot, group_types[g], b"", 0)
    return store


def decided(rows, exp, fired, cfg_dict, tmp_dir):
    """rows the text rules decide -- the reference differs from the reference of the config with the rules
    removed -- in all and per form removed (exclude_info_types included).  exp / fired: the reference's
    result and the forms that dropped a candidate, per row; a row where none did has nothing to compare."""
    import text_excl_configs as TC
    import text_excl_ref as TR
    from oracle import pii_oracle as O

    def ref_without(name, forms):
        return TR.Ref(O.RuleConfig.load(TC.write(tmp_dir, "without_" + name, TR.without_text_rules(cfg_dict, forms))))
    refs = {"all": ref_without("all", TR.FORMS)}
    refs.update({f: ref_without(f, [f]) for f in TR.FORMS})
    refs["exclude_info_types"] = ref_without("types", ["exclude_info_types"])
    n = dict.fromkeys(refs, 0)
    for (_, _, text, _), x, f in zip(rows, exp, fired):
        if not f:
            continue
        for name, r in refs.items():
            if r.find_pii(text, x[2]) != x[1]:
                n[name] += 1
    return n


FILL = "lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et "


def cut_row():
    """one row of three 1 KiB lanes (as one row of a batch whose lanes are 1 KiB: the caller pads the batch)
    under text_excl_configs.hand(): an ORDER_ID tested by FULL_MATCH straddles the first lane boundary, a
    TICKET's hotword window (12 bytes before it) crosses the second -- the hotword in one lane, the match in
    the next.  Returns (row, positions of the two matches)."""
    def fill(n):
        return (FILL * (n // len(FILL) + 2))[:n - 1] + " "
    a = fill(1024 - 4) + "ORD-01234 "                       # bytes 1020..1029: four before the boundary
    assert len(a) == 1030
    b = fill(2048 - 7 - len(a)) + "sample TK12345 "         # "sample " ends at 2048, the ticket starts there
    row = a + b
    assert row[1020:1029] == "ORD-01234" and row[2041:2047] == "sample" and row[2048:2055] == "TK12345"
    row += fill(3000 - len(row)) + "ORD-51234 and TK54321 end"
    return row.encode(), (1020, 2048)


def window_convs():
    """conversations whose exclusion hotword window crosses a "\\n" join (text_excl_configs.hand(): TICKET,
    12 bytes before; BADGE, 6 bytes after), all CUSTOMER rows: (conv, role, text, ts)"""
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    convs = [
        [b"this is a sample", b"TK12345 is mine", b"and TK54321 too", b"BG1234", b"void", b"BG4321", b"x void"],
        [b"hello", b"ORD-01234 ORD-51234", b"sample", b"", b"TK00001", b"teal", b"BG1111"],
        [b"a Red car", b"BG7777", b" void", b"zip z00000-1234 ok", b"REF TST 123456", b"xzbb zbb", b"sample", b"TK99999"],
    ]
    return [(c, C, t, 1 + k) for c, conv in enumerate(convs) for k, t in enumerate(conv)]


if __name__ == "__main__":
    import tempfile
    import time
    import text_excl_configs as TC
    import text_excl_ref as TR
    from oracle import pii_oracle as O
    d = tempfile.mkdtemp()
    ref = TR.Ref(O.RuleConfig.load(TC.write(d, "hand", TC.hand())))
    for t, want in HAND:
        got = ref.redact(t)[0]
        print("ok " if got == want else "BAD", t, got, "" if got == want else want)
    ref = TR.Ref(O.RuleConfig.load(TC.write(d, "ctx", TC.context_cfg())))
    for t, ctx, want in CONTEXT:
        got = ref.redact(t, ctx)[0]
        print("ok " if got == want else "BAD", t, ctx, got, "" if got == want else want)
    path = TC.write(d, "all", TC.all_forms())
    ref = TR.Ref(O.RuleConfig.load(path))
    groups = [t for t, _, _ in pkg("compiler").Rules.load(path).kw_groups]
    rows, ctx = random_rows(groups)
    t0 = time.time()
    exp, fired = [], []
    store = oracle_store(ctx, groups)
    for row in rows:
        exp.append(ref.process_rows([row], store)[0])
        fired.append(ref.fired)
    t1 = time.time()
    print(len(rows), "rows, reference %.1f s; decided:" % (t1 - t0), decided(rows, exp, fired, TC.all_forms(), d),
          "%.1f s" % (time.time() - t1))
