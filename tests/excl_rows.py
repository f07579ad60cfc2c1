"""Rows for the general exclusion tests and what the oracle makes of them.

Template rows plant every way an excluder can lie against its victim under excl_configs.G1 (randomised
names and digits around the four known-answer rows), the shapes that must NOT exclude (touching spans, an
excluder in the neighbouring row), and synth bank rows in between.  exclusion_shapes() classifies, from
the oracle's own candidate list, which shapes fired in a row, so a parity test can show it is not vacuous.
No GPU here: `python tests/excl_rows.py` prints the counts."""
import random

from conftest import pkg

SHAPES = ("contained", "excluder_inside", "left_overlap", "right_overlap", "chain")
WORDS = ["please", "note", "the", "ticket", "about", "order", "thanks", "regarding", "update", "hello", "also", "so"]
NAMES = ["jane", "bob.smith", "a_lee", "kim", "zoe-w", "r2d2", "maria.g"]


def _ssn(r):
    return "%03d-%02d-%04d" % (r.choice([r.randrange(1, 666), r.randrange(667, 900)]), r.randrange(1, 100),
                               r.randrange(1, 10000))


def _phone(r, sep="-"):
    return "%d%02d%s%d%02d%s%04d" % (r.randrange(2, 10), r.randrange(100), sep, r.randrange(2, 10), r.randrange(100),
                                     sep, r.randrange(10000))


def _d(r, n):
    return "".join(r.choice("0123456789") for _ in range(n))


def _words(r, lo=0, hi=4):
    return " ".join(r.choice(WORDS) for _ in range(r.randrange(lo, hi + 1)))


def _wrap(r, core):
    a, b = _words(r), _words(r)
    return ((a + " ") if a else "") + core + ((" " + b) if b else "")


def _name(r):
    return r.choice(NAMES) + (_d(r, 2) if r.random() < 0.3 else "")


# each template: rng -> one row, or a list of consecutive rows
def t_email_allowed(r):          # excluder strictly inside the victim; the excluded e-mail excludes the handle (chain)
    return _wrap(r, "%s@%s.com" % (_name(r), r.choice(["acme", "example"])))


def t_email_other(r):            # no false exclusion
    return _wrap(r, "%s@%s" % (_name(r), r.choice(["acme.org", "example.net", "acme.co", "other.com"])))


def t_domain_alone(r):           # OUR_DOMAIN and SOCIAL_HANDLE on the same span: same start (G2: contained)
    return _wrap(r, "write to @%s.com" % r.choice(["acme", "example"]))


def t_tail_left(r):              # TAIL_REF starts before the phone number and ends inside it
    return _wrap(r, "%s %s#%s" % (_ssn(r), r.choice(["", " "]), _phone(r)))


def t_tail_right(r):             # TAIL_REF starts inside the phone number and ends past it
    return _wrap(r, "%s%s#%s" % (_phone(r, r.choice("-. ")), r.choice(["", " "]), _d(r, 3)))


def t_tail_touching(r):          # TAIL_REF ends where the phone number starts: must not exclude
    return _wrap(r, "%s %s#%s(%d%02d) %d%02d-%04d" % (r.choice(["ref", "no"]), _d(r, 4), _d(r, 3), r.randrange(2, 10),
                                                     r.randrange(100), r.randrange(2, 10), r.randrange(100),
                                                     r.randrange(10000)))


def t_pair3_skip(r):             # PAIR3's second start lies inside its first match: skipped, the SSN stays
    return _wrap(r, "%s %s %s" % (_d(r, 3), _d(r, 3), _ssn(r)))


def t_pair3_hit(r):              # PAIR3 overlaps the SSN's head
    return _wrap(r, "%s %s" % (_d(r, 3), _ssn(r)))


def t_pair3_in_phone(r):         # PAIR3 inside a phone number written with blanks: no rule between them
    return _wrap(r, _phone(r, " "))


def t_test_card(r):              # FULL entry: TEST_CARD on the card number's span (same start, same end)
    return _wrap(r, "card 4111%s1111%s1111%s1111" % ((r.choice(["", " ", "-"]),) * 3))


def t_other_card(r):             # a card number TEST_CARD does not match
    return _wrap(r, "card 4141 1212 2323 5009")


def t_next_row(r):               # the excluder in the NEXT row: must not exclude across rows
    return ["%s %s@acme.org" % (_words(r, 1, 3), _name(r)), "@acme.com %s" % _words(r, 1, 3)]


def t_prev_row(r):               # the excluder at the end of the PREVIOUS row
    return ["%s %s #%s" % (_words(r, 1, 3), _d(r, 4), _d(r, 3)),
            "(%d%02d) %d%02d-%04d %s" % (r.randrange(2, 10), r.randrange(100), r.randrange(2, 10), r.randrange(100),
                                         r.randrange(10000), _words(r, 1, 3))]


TEMPLATES = [t_email_allowed, t_email_other, t_domain_alone, t_tail_left, t_tail_right, t_tail_touching, t_pair3_skip,
             t_pair3_hit, t_pair3_in_phone, t_test_card, t_other_card, t_next_row, t_prev_row]


def template_texts(r, n):
    """about n rows, every template in turn"""
    out = []
    k = 0
    while len(out) < n:
        x = TEMPLATES[k % len(TEMPLATES)](r)
        out += [t.encode() for t in (x if isinstance(x, list) else [x])]
        k += 1
    return out


def parity_rows(group_types, n_rows=3000, seed=11):
    """rows (slot, role, text, ts) and the context each slot must hold before the call: slot 0 none, slot
    1 + g the context group g -- every context variant sees template and bank rows, all CUSTOMER rows"""
    from oracle import pii_oracle as O
    synth = pkg("synth")
    r = random.Random(seed)
    bank = [t for t in synth.build_bank(50, 600, seed=seed).texts]
    per = n_rows // (1 + len(group_types))
    rows, contexts = [], {}
    for slot in range(1 + len(group_types)):
        if slot:
            contexts[slot] = slot - 1
        texts = template_texts(r, (2 * per) // 3)
        texts += [r.choice(bank) for _ in range(per - len(texts))]
        # (template pairs stay adjacent: shuffle blocks of two)
        blocks = [texts[i:i + 2] for i in range(0, len(texts), 2)]
        r.shuffle(blocks)
        rows += [(slot, O.ROLE_CUSTOMER, t, 1000) for b in blocks for t in b]
    return rows, contexts


def oracle_store(contexts, group_types):
    from oracle import pii_oracle as O
    store = O.ContextStore()
    for slot, g in contexts.items():
        store.set(slot, group_types[g], b"", 0)
    return store


def candidates(text, cfg, expected):
    """find_pii's candidate list before exclusion (oracle/pii_oracle.py find_pii, up to the min_likelihood filter)"""
    from oracle import pii_oracle as O
    v = cfg.variant(expected)
    cands = []
    for det in cfg.detectors:
        if det.type_name not in v.enabled_types:
            continue
        for m in det.regex.finditer(text):
            s, e = m.span()
            if det.validator and not O.VALIDATORS[det.validator](text[s:e]):
                continue
            lik = det.likelihood
            for rs in v.rule_sets:
                if det.type_name in rs.types:
                    for h in rs.hotwords:
                        if h.hit(text, s, e):
                            lik = h.adjust(lik)
            cands.append(O.Finding(s, e, cfg.type_id[det.type_name], lik))
    return [c for c in cands if c.likelihood >= v.min_likelihood], v


def exclusion_shapes(text, cfg, expected):
    """the shapes (SHAPES) by which an exclusion fired in this row"""
    cands, v = candidates(text, cfg, expected)
    names = cfg.type_names
    hits, drop = [], set()
    for rs in v.rule_sets:
        for ex in rs.exclusions:
            for i, c in enumerate(cands):
                if names[c.type_id] not in rs.types:
                    continue
                for j, g in enumerate(cands):
                    if j == i or names[g.type_id] not in ex.exclude_types:
                        continue
                    if ex.matching == "MATCHING_TYPE_PARTIAL_MATCH":
                        hit = g.start < c.end and c.start < g.end
                    else:
                        hit = g.start <= c.start and c.end <= g.end
                    if hit:
                        hits.append((i, j))
                        drop.add(i)
    out = set()
    for i, j in hits:
        c, g = cands[i], cands[j]
        if g.start <= c.start and c.end <= g.end:
            out.add("contained")
        elif c.start <= g.start and g.end <= c.end:
            out.add("excluder_inside")
        elif g.start < c.start:
            out.add("left_overlap")
        else:
            out.add("right_overlap")
        if j in drop:
            out.add("chain")
    return out


def shape_counts(rows, exp, cfg):
    """rows in which each shape fired; exp = process_rows' result (its context type per row)"""
    n = dict.fromkeys(SHAPES, 0)
    for (_, _, text, _), x in zip(rows, exp):
        for s in exclusion_shapes(text, cfg, x[2]):
            n[s] += 1
    return n


# ------------------------------------------------------------------------------------------ cut rows
FILL = "lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et "
SNIPPETS = ["x jane@acme.com y", "536-22-1234 #212-555-0187 ok", "111 222 333-22-4444 ok"]


def cut_rows(seed=5):
    """<= 200 rows of 500-700 bytes (every one cut into 128-byte lanes in a batch this small).  Every
    snippet is planted at each of the 128 byte offsets modulo the lane size (batch relative), so whatever
    the lane boundaries' phase, each of its bytes falls next to a boundary in some row: the excluder and
    its victim, or an excluder and the earlier match that makes finditer skip it, in different lanes."""
    r = random.Random(seed)
    places = [(s, k) for s in SNIPPETS for k in range(128)]
    r.shuffle(places)

    def fill(n):
        out = (FILL * (n // len(FILL) + 2))[r.randrange(len(FILL)):][:n]
        return (out[:-1] + " ") if n else out

    rows, pos = [], 0
    for i in range(0, len(places), 2):
        row = ""
        for snip, k in places[i:i + 2]:
            pad = 20 + r.randrange(20)
            pad += (k - (pos + len(row) + pad)) % 128          # the snippet starts at offset k modulo 128
            row += fill(pad) + snip + " "
            row += fill(100 + r.randrange(20))
        row += fill(max(0, 500 - len(row)))
        assert 500 <= len(row) <= 700, len(row)
        rows.append(row.encode())
        pos += len(row)
    assert len(rows) <= 200
    return rows


if __name__ == "__main__":
    import os
    import tempfile
    import excl_configs as XC
    from oracle import pii_oracle as O
    d = tempfile.mkdtemp()
    for name in ("G1", "G2"):
        cfg = O.RuleConfig.load(XC.write(d, name, XC.CONFIGS[name]()))
        groups = [t for t, _, _ in pkg("compiler").Rules.load(os.path.join(d, name + ".json")).kw_groups]
        rows, ctx = parity_rows(groups)
        exp = O.process_rows(rows, cfg, oracle_store(ctx, groups))
        print(name, len(rows), "rows", shape_counts(rows, exp, cfg))
    cfg = O.RuleConfig.load(XC.write(d, "G1", XC.g1()))
    cr = cut_rows()
    print("cut rows", len(cr), min(map(len, cr)), max(map(len, cr)),
          {s: sum(1 for t in cr if s in exclusion_shapes(t, cfg, None)) for s in SHAPES})
