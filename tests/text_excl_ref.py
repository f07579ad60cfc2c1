"""The reference of the text exclusion tests: oracle.find_pii restated with exclusion_rule.regex,
.dictionary and .exclude_by_hotword (the oracle itself is frozen and ignores these forms), plus the
redaction, row replay and window wrappers the tests need.

A rule of a rule set applies to a candidate c = [s, e) whose type the rule set lists; quote = text[s:e]:
  regex / dictionary   FULL_MATCH (default): drop c if re.fullmatch(pat, quote); PARTIAL_MATCH: if
                       re.search(pat, quote); INVERSE_MATCH: if not re.fullmatch(pat, quote)
  exclude_by_hotword   drop c if HotwordRule.hit(text, s, e) of the oracle would be true
The rules mark candidates in the oracle's exclusion loop, over the unfiltered candidate list: a marked
candidate still excludes others through exclude_info_types (and was found by finditer, so its pattern's
next match starts after it); it only leaves before overlap resolution.

test_text_excl_ref.py pins this to oracle.find_pii on configs without such rules.  No GPU here."""
import re
from typing import List, Optional, Sequence

from oracle import pii_oracle as O

FULL, PARTIAL, INVERSE = "MATCHING_TYPE_FULL_MATCH", "MATCHING_TYPE_PARTIAL_MATCH", "MATCHING_TYPE_INVERSE_MATCH"
FORMS = ("regex", "dictionary", "exclude_by_hotword")


class TextRule:
    """one exclusion_rule of a text form; drops(text, s, e) -> bool"""

    def __init__(self, ex: dict):
        self.form = next(k for k in FORMS if k in ex)
        self.matching = ex.get("matching_type", FULL)
        if self.form == "regex":
            pat = ex["regex"]["pattern"]
        elif self.form == "dictionary":
            pat = r"(?i)\b(?:" + "|".join(re.escape(w) for w in ex["dictionary"]["word_list"]["words"]) + r")\b"
        else:
            hw = ex["exclude_by_hotword"]
            prox = hw.get("proximity", {})
            self.hot = O.HotwordRule(hw["hotword_regex"]["pattern"], int(prox.get("window_before", 0)),
                                     int(prox.get("window_after", 0)), None)
            return
        self.regex = re.compile(pat.encode("ascii"))

    def drops(self, text: bytes, s: int, e: int) -> bool:
        if self.form == "exclude_by_hotword":
            return self.hot.hit(text, s, e)
        quote = text[s:e]
        if self.matching == PARTIAL:
            return self.regex.search(quote) is not None
        full = self.regex.fullmatch(quote) is not None
        return full if self.matching == FULL else not full


def is_text_rule(rule: dict) -> bool:
    return "exclusion_rule" in rule and any(k in rule["exclusion_rule"] for k in FORMS)


def without_text_rules(cfg: dict, forms: Sequence[str] = FORMS) -> dict:
    """the config with its exclusion rules of the given text forms removed (everything else kept)"""
    import copy
    out = copy.deepcopy(cfg)
    for rs in out.get("inspect_config", {}).get("rule_set", []) or []:
        rs["rules"] = [r for r in rs.get("rules", [])
                       if not ("exclusion_rule" in r and any(k in r["exclusion_rule"] for k in forms))]
    return out


class Ref:
    """find_pii and its wrappers over one config (the oracle's RuleConfig of the same file)"""

    def __init__(self, ocfg: O.RuleConfig):
        self.cfg = ocfg
        self._sets = {}
        self.fired = frozenset()      # forms whose rules dropped a candidate in the last find_pii call

    def rule_sets(self, expected_type: Optional[str]):
        """per rule set of the variant, in order: (types, exclude_info_types rules, text rules)"""
        if expected_type not in self._sets:
            insp, _ = self.cfg.merged_inspect_config(expected_type)
            out = []
            for rs in insp.get("rule_set") or []:
                types = tuple(it.get("name") for it in rs.get("info_types", []))
                by_type, by_text = [], []
                for rule in rs.get("rules", []):
                    if is_text_rule(rule):
                        by_text.append(TextRule(rule["exclusion_rule"]))
                    elif "exclusion_rule" in rule:
                        ex = rule["exclusion_rule"]
                        names = tuple(it["name"] for it in ex.get("exclude_info_types", {}).get("info_types", []))
                        by_type.append((names, ex.get("matching_type", FULL)))
                out.append((types, by_type, by_text))
            self._sets[expected_type] = out
        return self._sets[expected_type]

    def find_pii(self, text: bytes, expected_type: Optional[str] = None) -> List[O.Finding]:
        cfg = self.cfg
        v = cfg.variant(expected_type)
        cands: List[O.Finding] = []
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
        cands = [c for c in cands if c.likelihood >= v.min_likelihood]
        names = cfg.type_names
        drop, fired = set(), set()
        for types, by_type, by_text in self.rule_sets(expected_type):
            for i, c in enumerate(cands):
                if names[c.type_id] not in types:
                    continue
                for ex_types, matching in by_type:
                    for j, g in enumerate(cands):               # every candidate, dropped or not
                        if j == i or names[g.type_id] not in ex_types:
                            continue
                        if matching == PARTIAL:
                            hit = g.start < c.end and c.start < g.end
                        else:
                            hit = g.start <= c.start and c.end <= g.end
                        if hit:
                            drop.add(i)
                            break
                for r in by_text:
                    if r.drops(text, c.start, c.end):
                        drop.add(i)
                        fired.add(r.form)
        self.fired = frozenset(fired)
        cands = [c for i, c in enumerate(cands) if i not in drop]
        cands.sort(key=lambda c: (c.start, -(c.end - c.start), -c.likelihood, c.type_id))
        kept, max_end = [], -1
        for c in cands:
            if c.start >= max_end:
                kept.append(c)
                max_end = c.end
        return kept

    def redact(self, text: bytes, expected_type: Optional[str] = None):
        fs = self.find_pii(text, expected_type)
        return O.apply_redaction(text, fs, self.cfg), fs

    def process_rows(self, rows, store: Optional[O.ContextStore] = None):
        """oracle.process_rows with this find_pii: (redacted, findings, context type used, context stored)"""
        store = store if store is not None else O.ContextStore()
        out = []
        for conv, role, text, ts in rows:
            if role == O.ROLE_AGENT:
                red, fs = self.redact(text, None)
                et = O.extract_expected_pii(text, self.cfg)
                if et:
                    store.set(conv, et, text, ts)
                out.append((red, fs, None, et))
            elif role == O.ROLE_CUSTOMER:
                ctx = store.get(conv, ts)
                et = ctx[0] if ctx else None
                red, fs = self.redact(text, et)
                out.append((red, fs, et, None))
            else:
                red, fs = self.redact(text, None)
                out.append((red, fs, None, None))
        return out

    def process_window_rows(self, rows, n: int = 5, store: Optional[O.ContextStore] = None):
        """oracle.process_window_rows with this find_pii: (redacted window, findings, context type used)"""
        store = store if store is not None else O.ContextStore()
        history = {}
        out = []
        for conv, role, text, ts in rows:
            if role == O.ROLE_AGENT:
                et = O.extract_expected_pii(text, self.cfg)
                if et:
                    store.set(conv, et, text, ts)
            win = history.setdefault(conv, [])
            win.append(text)
            del win[:-n]
            ctx = store.get(conv, ts)
            et = ctx[0] if ctx else None
            red, fs = self.redact(b"\n".join(win), et)
            out.append((red, fs, et))
        return out
