"""Host rule compiler: dlp_config.yaml (+ build-defined built-ins) -> DFA tables -> rules blob.

Replaces what Google Cloud DLP does internally with ``inspect_config`` (dlp_config.yaml:92-194) and
with the context branch of ``call_dlp_for_redaction`` (main_service/main.py:609-686).

Regexes are parsed with the standard library's own ``sre_parse`` (the parser ``re`` uses), as BYTES
patterns, so the engine and the CPU oracle start from the same syntax tree.  Three DFA families are
built from a Thompson NFA with explicit assertion nodes (``\\b``, ``\\B``, ``\\A``/``^``, ``\\Z``):

* SCAN   - one REVERSE, unanchored, set-semantics DFA over every detector pattern and every
           context-keyword group.  The HIP scan kernel walks each utterance right-to-left through it;
           entering a state whose accept list is non-empty means "a match of these patterns STARTS
           here".  It is the only dense, per-byte table (LDS-resident).
* FIRST  - per detector pattern, an ANCHORED leftmost-first (priority-ordered, RE2-style) forward
           DFA.  Run from a start found by SCAN it returns exactly the end ``re`` would return.
* HOT    - per hotword rule, an unanchored set-semantics forward DFA run over the proximity window
           (window edges behave as text edges, like ``re.search(text[lo:hi])``).

Assertions are resolved with one character of look-ahead: a DFA state is (core NFA set, kind of the
previous character); closures are taken with the kind of the NEXT character known, so acceptance is
reported one step late, as a property of the state entered (see DESIGN.md §DFA encoding).
"""
from __future__ import annotations

import base64
import hashlib
import io
import json
import os
import dataclasses
import re
import struct
import sys
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import yaml

if sys.version_info >= (3, 11):                               # pragma: no cover
    from re import _constants as C
    from re import _parser as sre_parse
else:
    import sre_constants as C
    import sre_parse

HERE = os.path.dirname(os.path.abspath(__file__))
RULES_DIR = os.path.join(HERE, "rules")

LIKELIHOOD = {"LIKELIHOOD_UNSPECIFIED": 0, "VERY_UNLIKELY": 1, "UNLIKELY": 2, "POSSIBLE": 3,
              "LIKELY": 4, "VERY_LIKELY": 5}
VERY_LIKELY = 5
DEFAULT_MIN_LIKELIHOOD = 3
VALIDATOR_IDS = {None: 0, "luhn": 1, "nanp": 2, "ssn": 3, "ein": 4, "ipv4": 5, "swift": 6, "iban": 7}
BLOB_MAGIC = b"PIIRULE1"
PSEUDO_GROUP_MAX_TYPES = 64     # rule sets up to this many types get a context variant per type


class RuleError(ValueError):
    pass


def lik_value(x) -> int:
    return x if isinstance(x, int) else LIKELIHOOD[str(x)]


# ============================================================================ character sets ====
ALL = (1 << 256) - 1
DIGIT = sum(1 << c for c in range(48, 58))
WORD = DIGIT | sum(1 << c for c in range(65, 91)) | sum(1 << c for c in range(97, 123)) | (1 << 95)
SPACE = sum(1 << c for c in (9, 10, 11, 12, 13, 32))
NEWLINE = 1 << 10
UPPER = sum(1 << c for c in range(65, 91))
LOWER = sum(1 << c for c in range(97, 123))


def fold(cs: int) -> int:
    """ASCII case closure (IGNORECASE on bytes patterns)."""
    return cs | ((cs & UPPER) << 32) | ((cs & LOWER) >> 32)


_CATEGORIES = {
    C.CATEGORY_DIGIT: DIGIT, C.CATEGORY_NOT_DIGIT: ALL & ~DIGIT,
    C.CATEGORY_WORD: WORD, C.CATEGORY_NOT_WORD: ALL & ~WORD,
    C.CATEGORY_SPACE: SPACE, C.CATEGORY_NOT_SPACE: ALL & ~SPACE,
}

# assertion kinds (forward sense); the reverse NFA swaps BEGIN <-> END
A_BOUNDARY, A_NONBOUNDARY, A_BEGIN, A_END = range(4)
# character kinds: BOT (no previous char), W word char, N non-word char, EOT (no next char)
K_BOT, K_W, K_N, K_EOT = 0, 1, 2, 3


def assert_ok(kind: int, pk: int, nk: int) -> bool:
    if kind == A_BOUNDARY or kind == A_NONBOUNDARY:
        b = (pk == K_W) != (nk == K_W)
        return b if kind == A_BOUNDARY else not b
    if kind == A_BEGIN:
        return pk == K_BOT
    return nk == K_EOT


# ======================================================================================= NFA ====
CHAR, SPLIT, EPS, ASSERT, MATCH = range(5)


class NFA:
    def __init__(self):
        self.kind: List[int] = []
        self.a: List[int] = []      # CHAR/EPS/ASSERT: next ; SPLIT: preferred ; MATCH: pattern id
        self.b: List[int] = []      # SPLIT: other ; ASSERT: assertion kind
        self.cs: List[int] = []     # CHAR: byte set

    def add(self, kind, a=-1, b=-1, cs=0) -> int:
        self.kind.append(kind)
        self.a.append(a)
        self.b.append(b)
        self.cs.append(cs)
        return len(self.kind) - 1


def parse(pattern: str):
    try:
        return sre_parse.parse(pattern.encode("ascii") if isinstance(pattern, str) else pattern, 0)
    except Exception as e:  # pragma: no cover - surfaced to the caller
        raise RuleError(f"cannot parse regex {pattern!r}: {e}")


def _items_nullable(items) -> bool:
    return all(_nullable(op, av) for op, av in items)


def _nullable(op, av) -> bool:
    if op in (C.LITERAL, C.NOT_LITERAL, C.ANY, C.IN):
        return False
    if op == C.AT:
        return True
    if op == C.SUBPATTERN:
        return _items_nullable(av[-1])
    if op == C.BRANCH:
        return any(_items_nullable(b) for b in av[1])
    if op in (C.MAX_REPEAT, C.MIN_REPEAT):
        return av[0] == 0 or _items_nullable(av[2])
    raise RuleError(f"unsupported regex construct {op}")


class Emitter:
    """Thompson construction by continuation: emit(items, cont) returns the entry node."""

    def __init__(self, nfa: NFA, reverse: bool):
        self.nfa = nfa
        self.reverse = reverse

    def charset(self, op, av, flags) -> int:
        ic = flags & C.SRE_FLAG_IGNORECASE
        if op == C.LITERAL:
            cs = 1 << av
            return fold(cs) if ic else cs
        if op == C.NOT_LITERAL:
            cs = 1 << av
            return ALL & ~(fold(cs) if ic else cs)
        if op == C.ANY:
            return ALL if flags & C.SRE_FLAG_DOTALL else ALL & ~NEWLINE
        if op == C.IN:
            cs, neg = 0, False
            for iop, iav in av:
                if iop == C.NEGATE:
                    neg = True
                elif iop == C.LITERAL:
                    cs |= 1 << iav
                elif iop == C.RANGE:
                    lo, hi = iav
                    cs |= ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)
                elif iop == C.CATEGORY:
                    cs |= _CATEGORIES[iav]
                else:
                    raise RuleError(f"unsupported class item {iop}")
            if ic:
                cs = fold(cs)
            return (ALL & ~cs) if neg else cs
        raise AssertionError(op)

    def emit(self, items, flags, cont) -> int:
        seq = list(items)
        if not self.reverse:
            seq = seq[::-1]
        for op, av in seq:          # build back to front: each item continues into `cont`
            cont = self.emit_one(op, av, flags, cont)
        return cont

    def emit_one(self, op, av, flags, cont) -> int:
        n = self.nfa
        if op in (C.LITERAL, C.NOT_LITERAL, C.ANY, C.IN):
            return n.add(CHAR, cont, cs=self.charset(op, av, flags))
        if op == C.SUBPATTERN:
            _group, add_f, del_f, sub = av
            if add_f & C.SRE_FLAG_MULTILINE:
                raise RuleError("MULTILINE is not supported")
            return self.emit(sub, (flags | add_f) & ~del_f, cont)
        if op == C.BRANCH:
            alts = [self.emit(b, flags, cont) for b in av[1]]
            entry = alts[-1]
            for alt in reversed(alts[:-1]):
                entry = n.add(SPLIT, alt, entry)
            return entry
        if op in (C.MAX_REPEAT, C.MIN_REPEAT):
            lo, hi, sub = av
            greedy = op == C.MAX_REPEAT
            if _items_nullable(sub) and hi != lo:
                raise RuleError("repeat of a sub-pattern that can match empty is not supported")
            if hi == C.MAXREPEAT:
                loop = n.add(SPLIT)
                body = self.emit(sub, flags, loop)
                if greedy:
                    n.a[loop], n.b[loop] = body, cont
                else:
                    n.a[loop], n.b[loop] = cont, body
                tail = loop
            else:
                tail = cont
                for _ in range(hi - lo):
                    body = self.emit(sub, flags, tail)
                    tail = n.add(SPLIT, body, cont) if greedy else n.add(SPLIT, cont, body)
            for _ in range(lo):
                tail = self.emit(sub, flags, tail)
            return tail
        if op == C.AT:
            if av in (C.AT_BOUNDARY,):
                k = A_BOUNDARY
            elif av == C.AT_NON_BOUNDARY:
                k = A_NONBOUNDARY
            elif av in (C.AT_BEGINNING, C.AT_BEGINNING_STRING):
                k = A_BEGIN
            elif av == C.AT_END_STRING:
                k = A_END
            else:
                raise RuleError("'$' / MULTILINE anchors are not supported (use \\Z)")
            if self.reverse and k in (A_BEGIN, A_END):
                k = A_END if k == A_BEGIN else A_BEGIN
            return n.add(ASSERT, cont, k)
        raise RuleError(f"unsupported regex construct {op}")


def add_pattern(nfa: NFA, pattern: str, pid: int, reverse: bool) -> int:
    tree = parse(pattern)
    flags = tree.state.flags
    if flags & C.SRE_FLAG_MULTILINE:
        raise RuleError("MULTILINE is not supported")
    if _items_nullable(list(tree)):
        raise RuleError(f"pattern {pattern!r} can match the empty string")
    m = nfa.add(MATCH, pid)
    return Emitter(nfa, reverse).emit(list(tree), flags, m)


def add_whole(nfa: NFA, pattern: str, pid: int) -> int:
    r"""`\A(?:pattern)\Z`, built on the parsed tree (the pattern's global flags stay where they are):
    run unanchored over a text it accepts iff re.fullmatch(pattern, text) -- existence of a match of the
    whole text, whatever the alternation order."""
    tree = parse(pattern)
    flags = tree.state.flags
    if flags & C.SRE_FLAG_MULTILINE:
        raise RuleError("MULTILINE is not supported")
    if _items_nullable(list(tree)):
        raise RuleError(f"pattern {pattern!r} can match the empty string")
    m = nfa.add(MATCH, pid)
    items = [(C.AT, C.AT_BEGINNING_STRING)] + list(tree) + [(C.AT, C.AT_END_STRING)]
    return Emitter(nfa, False).emit(items, flags, m)


# ================================================================================ byte classes ==
def byte_classes(nfa: NFA) -> Tuple[np.ndarray, List[int]]:
    """Coarsest partition of 0..255 respecting every CHAR set and the word-character set."""
    blocks = [ALL]
    sets = {WORD, NEWLINE}
    sets.update(cs for k, cs in zip(nfa.kind, nfa.cs) if k == CHAR)
    for s in sets:
        nb = []
        for b in blocks:
            x, y = b & s, b & ~s
            if x:
                nb.append(x)
            if y:
                nb.append(y)
        blocks = nb
    cmap = np.zeros(256, dtype=np.uint8)
    reps = []
    blocks.sort(key=lambda b: (b & -b).bit_length())   # order classes by smallest member
    for ci, b in enumerate(blocks):
        reps.append((b & -b).bit_length() - 1)
        for c in range(256):
            if (b >> c) & 1:
                cmap[c] = ci
    if len(blocks) > 255:
        raise RuleError("too many byte classes")
    return cmap, reps


def _kind_of_byte(c: int) -> int:
    return K_W if (WORD >> c) & 1 else K_N


# ================================================================================== DFA core ====
@dataclass
class DFA:
    cmap: np.ndarray                 # uint8[256] byte -> class
    trans: np.ndarray                # uint16[S, C+1]; column C = end-of-text pseudo-class
    flags: np.ndarray                # uint8[S]
    start: List[int]                 # start state per previous-character kind (BOT, W, N)
    accept: List[Tuple[int, ...]] = field(default_factory=list)   # set DFAs: pattern ids per state

    @property
    def n_states(self):
        return self.trans.shape[0]

    @property
    def n_classes(self):
        return self.trans.shape[1] - 1


def _closure_set(nfa: NFA, seeds, pk, nk):
    kind, a, b = nfa.kind, nfa.a, nfa.b
    chars, matches, seen, stack = [], [], set(), list(seeds)
    while stack:
        s = stack.pop()
        if s in seen:
            continue
        seen.add(s)
        k = kind[s]
        if k == CHAR:
            chars.append(s)
        elif k == MATCH:
            matches.append(a[s])
        elif k == SPLIT:
            stack.append(a[s])
            stack.append(b[s])
        elif k == EPS:
            stack.append(a[s])
        elif assert_ok(b[s], pk, nk):
            stack.append(a[s])
    return chars, frozenset(matches)


def _closure_ordered(nfa: NFA, seeds, pk, nk):
    kind, a, b = nfa.kind, nfa.a, nfa.b
    out, seen = [], set()
    for seed in seeds:
        stack = [seed]
        while stack:
            s = stack.pop()
            if s in seen:
                continue
            seen.add(s)
            k = kind[s]
            if k == CHAR or k == MATCH:
                out.append(s)
            elif k == SPLIT:
                stack.append(b[s])          # lower priority explored after the preferred branch
                stack.append(a[s])
            elif k == EPS:
                stack.append(a[s])
            elif assert_ok(b[s], pk, nk):
                stack.append(a[s])
    return out


def build_set_dfa(nfa: NFA, starts: Sequence[int], unanchored: bool, max_states: int = 60000) -> DFA:
    """Set-semantics DFA.  State key = (core, prev kind, accept set); accept set = patterns whose
    match ENDS right before the character just consumed (reported one step late)."""
    cmap, reps = byte_classes(nfa)
    ncls = len(reps)
    ckind = [_kind_of_byte(r) for r in reps]
    start_set = frozenset(starts)
    index: Dict[tuple, int] = {}
    keys: List[tuple] = []

    def sid(key):
        if key not in index:
            if len(keys) >= max_states:
                raise RuleError(f"DFA exceeds {max_states} states")
            index[key] = len(keys)
            keys.append(key)
        return index[key]

    empty = frozenset()
    starts_by_kind = []
    for pk in (K_BOT, K_W, K_N):
        starts_by_kind.append(sid((empty if unanchored else start_set, pk, empty)))
    rows = []
    i = 0
    while i < len(keys):
        core, pk, _acc = keys[i]
        row = [0] * (ncls + 1)
        seeds = (core | start_set) if unanchored else core
        if not seeds:                                    # anchored dead state
            row = [i] * (ncls + 1)
            rows.append(row)
            i += 1
            continue
        clos = {}
        for nk in (K_W, K_N, K_EOT):
            clos[nk] = _closure_set(nfa, seeds, pk, nk)
        for c in range(ncls):
            chars, acc = clos[ckind[c]]
            r = reps[c]
            nxt = frozenset(nfa.a[s] for s in chars if (nfa.cs[s] >> r) & 1)
            if not unanchored and not nxt:
                key = (empty, K_N, acc)
            else:
                key = (nxt, ckind[c], acc)
            row[c] = sid(key)
        _, acc = clos[K_EOT]
        row[ncls] = sid((empty, K_EOT, acc))
        rows.append(row)
        i += 1
    trans = np.array(rows, dtype=np.int64)
    accept = [tuple(sorted(k[2])) for k in keys]
    flags = np.array([1 if acc else 0 for acc in accept], dtype=np.uint8)
    dfa = DFA(cmap, trans, flags, starts_by_kind, accept)
    return minimize(dfa)


def relax_items(items, budget: int, skip_groups: bool = False):
    """Prefix relaxation for the SCAN prefilter: a pattern whose language, for every match of the
    original starting at s, has a match starting at s too (so SCAN reports a SUPERSET of starts;
    the exact FIRST DFA confirms each).  Bounded repeats are widened ({lo,hi} -> {min(lo,k)} X*),
    the sequence is cut after `budget` consuming characters, an alternation ends the prefix.
    An optional or starred group of several items ends the prefix where it stands; with `skip_groups`
    (add_relaxed: when that leaves nothing that consumes a character) it becomes the alternation of
    its relaxed body and the relaxed rest of the sequence, and the prefix ends after that.  The rest is
    what follows inside the enclosing group; a group that sets or clears a flag is not opened, so a pattern
    whose optional group ends such a group before any required character, (?i:(?:ab)?)c, is still refused."""
    out = []
    for i, (op, av) in enumerate(items):
        if op == C.AT:
            out.append((op, av))
            continue
        if budget <= 0:
            return out, False, 0
        if op in (C.LITERAL, C.NOT_LITERAL, C.ANY, C.IN):
            out.append((op, av))
            budget -= 1
            continue
        if op == C.SUBPATTERN:
            if skip_groups and not av[1] and not av[2]:
                # a group that changes no flag is its items in place, so that an optional group that ends it
                # still has a rest: ((?:ab)?)c\d
                r = relax_items(list(av[-1]) + list(items[i + 1:]), budget, True)
                return out + r[0], r[1], r[2]
            sub, full, budget = relax_items(list(av[-1]), budget, skip_groups)
            out.append((op, (av[0], av[1], av[2], sub)))
            if not full:
                return out, False, 0
            continue
        if op == C.BRANCH:
            # each alternative relaxed with the budget left; when every one of them is taken whole, the
            # prefix goes on past the alternation (with the smallest budget any alternative left), so a
            # pattern like (0?[1-9]|1[0-2])/... keeps its '/' instead of firing at every number
            rs = [relax_items(list(b), budget, skip_groups) for b in av[1]]
            out.append((op, (None, [r[0] for r in rs])))
            if not all(r[1] for r in rs):
                return out, False, 0
            budget = min(r[2] for r in rs)
            continue
        if op in (C.MAX_REPEAT, C.MIN_REPEAT):
            lo, hi, sub = av
            sub = list(sub)
            single = len(sub) == 1 and sub[0][0] in (C.LITERAL, C.NOT_LITERAL, C.ANY, C.IN)
            if not single:
                if lo == 0:
                    if skip_groups:
                        # one repetition or more begins with the body, none with what follows the group
                        out.append((C.BRANCH, (None, [relax_items(sub, budget, True)[0],
                                                      relax_items(list(items[i + 1:]), budget, True)[0]])))
                    return out, False, 0
                for _ in range(lo):
                    s2, full, budget = relax_items(sub, budget, skip_groups)
                    out.extend(s2)
                    if not full:
                        return out, False, 0
                if hi != lo:
                    return out, False, 0
                continue
            if hi != lo and hi != C.MAXREPEAT and hi <= budget and all(o == C.AT for o, _ in items[i + 1:]):
                # a bounded repeat that ends the sequence and fits whole is kept exact, so the trailing
                # assertion still filters -- \b\d{3,4}\b no longer fires at every longer digit run
                # (inside a sequence, widening spends only `lo` of the budget on it: more of what
                # follows is kept, e.g. IP_ADDRESS's dots)
                out.extend(sub * lo)
                out.append((C.MAX_REPEAT, (0, hi - lo, sub)))
                budget -= hi
                continue
            n = min(lo, budget)
            out.extend(sub * n)
            budget -= n
            if n < lo:
                return out, False, 0
            if hi != lo:
                out.append((C.MAX_REPEAT, (0, C.MAXREPEAT, sub)))
            continue
        raise RuleError(f"unsupported regex construct {op}")
    return out, True, budget


def add_relaxed(nfa: NFA, pattern: str, pid: int, budget: int, reverse: bool) -> int:
    tree = parse(pattern)
    items = list(tree)
    if budget > 0:
        items = relax_items(items, budget)[0]
        if _items_nullable(items):
            # the prefix ended at an optional group before any required character: (?:\+1[ -])?\d{3}-\d{4}
            items = relax_items(list(tree), budget, skip_groups=True)[0]
    if _items_nullable(items):
        raise RuleError(f"relaxed pattern of {pattern!r} can match the empty string")
    m = nfa.add(MATCH, pid)
    return Emitter(nfa, reverse).emit(items, tree.state.flags, m)


@dataclass
class MealyDFA:
    cmap: np.ndarray          # uint8[256]
    trans: np.ndarray         # uint16[S, C+1]; bit 15 set = this transition reports accepts
    start: int                # state at the right end of an utterance (reverse scan)
    acc_id: np.ndarray        # int32[S, C+1]: index into acc_sets (0 = none)
    acc_sets: List[Tuple[int, ...]]

    @property
    def n_states(self):
        return self.trans.shape[0]

    @property
    def n_classes(self):
        return self.trans.shape[1] - 1


def build_mealy_dfa(nfa: NFA, starts: Sequence[int], max_states: int = 32767,
                    max_bytes: Optional[int] = None) -> MealyDFA:
    """Unanchored set-semantics DFA with accepts on TRANSITIONS.  Transition (q, c) reports the
    patterns whose match ends right before c in scan direction (for the reverse SCAN: whose match
    STARTS right after c in text order).  `max_bytes` bounds the u16 table (rows padded to an even
    class count) and fails early (RuleError) when the subset construction exceeds it."""
    cmap, reps = byte_classes(nfa)
    ncls = len(reps)
    if max_bytes is not None:
        max_states = min(max_states, max_bytes // (2 * ((ncls + 2) & ~1)) * 2)
    ckind = [_kind_of_byte(r) for r in reps]
    start_set = frozenset(starts)
    index: Dict[tuple, int] = {}
    keys: List[tuple] = []

    def sid(key):
        if key not in index:
            if len(keys) >= max_states:
                raise RuleError(f"SCAN DFA exceeds {max_states} states")
            index[key] = len(keys)
            keys.append(key)
        return index[key]

    sid((frozenset(), K_BOT))
    acc_index: Dict[frozenset, int] = {frozenset(): 0}
    acc_sets: List[Tuple[int, ...]] = [()]
    rows, arows = [], []
    i = 0
    while i < len(keys):
        core, pk = keys[i]
        seeds = core | start_set
        clos = {nk: _closure_set(nfa, seeds, pk, nk) for nk in (K_W, K_N, K_EOT)}
        row, arow = [0] * (ncls + 1), [0] * (ncls + 1)
        for c in range(ncls + 1):
            if c == ncls:
                chars, acc = clos[K_EOT]
                row[c] = sid((frozenset(), K_EOT))
            else:
                chars, acc = clos[ckind[c]]
                r = reps[c]
                row[c] = sid((frozenset(nfa.a[s] for s in chars if (nfa.cs[s] >> r) & 1), ckind[c]))
            if acc:
                if acc not in acc_index:
                    acc_index[acc] = len(acc_sets)
                    acc_sets.append(tuple(sorted(acc)))
                arow[c] = acc_index[acc]
        rows.append(row)
        arows.append(arow)
        i += 1
    trans = np.array(rows, dtype=np.int64)
    accid = np.array(arows, dtype=np.int64)
    # Moore-style refinement on (target block, accept id) per column
    block = np.zeros(len(keys), dtype=np.int64)
    nblocks = 1
    while True:
        sig = np.concatenate([block[:, None], block[trans], accid], axis=1)
        _, nb = np.unique(sig, axis=0, return_inverse=True)
        nb = nb.reshape(-1)
        n = int(nb.max()) + 1
        if n == nblocks:
            break
        block, nblocks = nb, n
    rep = {}
    for s in range(len(keys)):
        rep.setdefault(int(block[s]), s)
    order = sorted(rep.keys(), key=lambda b: rep[b])
    newid = {b: j for j, b in enumerate(order)}
    t2 = np.zeros((nblocks, ncls + 1), dtype=np.uint16)
    a2 = np.zeros((nblocks, ncls + 1), dtype=np.int32)
    for b in order:
        s = rep[b]
        j = newid[b]
        t2[j] = [newid[int(block[t])] for t in trans[s]]
        a2[j] = accid[s]
    if nblocks >= 32768:
        raise RuleError("SCAN DFA too large for 15-bit state ids")
    t2 = t2 | np.where(a2 > 0, 0x8000, 0).astype(np.uint16)
    return MealyDFA(cmap, t2, newid[int(block[0])], a2, acc_sets)


def build_first_dfa(nfa: NFA, start: int, max_states: int = 60000) -> DFA:
    """Anchored leftmost-first DFA (RE2 'first match' construction).  flags bit0: a match ended
    right before the character just consumed; bit1: terminal (no thread left)."""
    cmap, reps = byte_classes(nfa)
    ncls = len(reps)
    ckind = [_kind_of_byte(r) for r in reps]
    index: Dict[tuple, int] = {}
    keys: List[tuple] = []

    def sid(key):
        if key not in index:
            if len(keys) >= max_states:
                raise RuleError(f"DFA exceeds {max_states} states")
            index[key] = len(keys)
            keys.append(key)
        return index[key]

    starts_by_kind = [sid(((start,), pk, 0)) for pk in (K_BOT, K_W, K_N)]
    rows = []
    i = 0
    while i < len(keys):
        core, pk, _m = keys[i]
        row = [0] * (ncls + 1)
        if not core:
            rows.append([i] * (ncls + 1))
            i += 1
            continue
        clos = {}
        for nk in (K_W, K_N, K_EOT):
            leaves = _closure_ordered(nfa, core, pk, nk)
            m = 0
            for j, s in enumerate(leaves):
                if nfa.kind[s] == MATCH:
                    leaves = leaves[:j]
                    m = 1
                    break
            clos[nk] = (leaves, m)
        for c in range(ncls):
            leaves, m = clos[ckind[c]]
            r = reps[c]
            nxt, seen = [], set()
            for s in leaves:
                if (nfa.cs[s] >> r) & 1:
                    t = nfa.a[s]
                    if t not in seen:
                        seen.add(t)
                        nxt.append(t)
            row[c] = sid((tuple(nxt), ckind[c] if nxt else K_N, m))
        leaves, m = clos[K_EOT]
        row[ncls] = sid(((), K_N, m))
        rows.append(row)
        i += 1
    trans = np.array(rows, dtype=np.int64)
    flags = np.array([(k[2] & 1) | (2 if not k[0] else 0) for k in keys], dtype=np.uint8)
    dfa = DFA(cmap, trans, flags, starts_by_kind, [])
    return minimize(dfa)


# ------------------------------------------------------------------- absorbed match starts ------
# A pattern  X{lo,} . rest  whose head is a greedy, unbounded repeat of ONE character class matches at
# s - 1 whenever it matches at s and text[s-1] is in X, with the same end (the head backtracks through
# the same positions), so finditer skips the start s as inside the previous match -- unless an earlier
# match of the pattern ends exactly at s, where finditer resumes.  A match can end at s only if
# text[s-1] is in Z (the bytes a match can end with) and text[s] is not in G (the class of a trailing
# greedy unbounded repeat, which would have taken it).  So the start s > 0 is dropped, before its
# FIRST run, iff
#     text[s-1] in X  and not (text[s-1] in Z and text[s] not in G)
# ("absorbed match starts").  Z may be a superset and G a subset: both only keep more.
_CLASS_OPS = (C.LITERAL, C.NOT_LITERAL, C.ANY, C.IN)


def _unbounded_class_repeat(op, av, flags) -> Optional[int]:
    """The class of a greedy `class{lo,}` item, else None."""
    if op != C.MAX_REPEAT or av[1] != C.MAXREPEAT:
        return None
    sub = list(av[2])
    if len(sub) != 1 or sub[0][0] not in _CLASS_OPS:
        return None
    return Emitter(None, False).charset(sub[0][0], sub[0][1], flags)


def _last_bytes(items, flags) -> int:
    """Superset of the bytes a non-empty match of the sequence `items` can end with."""
    cs = 0
    for op, av in reversed(list(items)):
        if op in _CLASS_OPS:
            cs |= Emitter(None, False).charset(op, av, flags)
        elif op == C.AT:
            pass
        elif op == C.SUBPATTERN:
            _group, add_f, del_f, sub = av
            cs |= _last_bytes(sub, (flags | add_f) & ~del_f)
        elif op == C.BRANCH:
            for b in av[1]:
                cs |= _last_bytes(b, flags)
        elif op in (C.MAX_REPEAT, C.MIN_REPEAT):
            cs |= _last_bytes(av[2], flags)
        else:
            return ALL
        if not _nullable(op, av):
            break
    return cs


def first_drop_sets(pattern) -> Optional[Tuple[int, int, int]]:
    """(X, Z, G) as byte sets when `pattern` is a top-level sequence that begins with a greedy,
    unbounded repeat of one character class (no assertion before it); None when not eligible."""
    tree = parse(pattern)
    items = list(tree)
    flags = tree.state.flags
    if not items:
        return None
    x = _unbounded_class_repeat(items[0][0], items[0][1], flags)
    if not x:
        return None
    g = _unbounded_class_repeat(items[-1][0], items[-1][1], flags) or 0
    return x, _last_bytes(items, flags), g


def first_drop(sets: Tuple[int, int, int], prev: int, cur: int) -> bool:
    """The rule above for one start: `prev` = text[s-1], `cur` = text[s] (s > 0)."""
    x, z, g = sets
    return bool((x >> prev) & 1) and not ((z >> prev) & 1 and not (g >> cur) & 1)


def drop_start(sets: Optional[Tuple[int, int, int]], text: bytes, s: int) -> bool:
    """Whether the start s of text is dropped (s == 0 and patterns that are not eligible: never)."""
    return sets is not None and 0 < s < len(text) and first_drop(sets, text[s - 1], text[s])


def add_first_drop(dfa: DFA, sets: Tuple[int, int, int]) -> Tuple[DFA, int]:
    """The rule as extra states of a FIRST DFA: a PRE state whose row maps the class of text[s-1] to
    the state the run from s starts in -- the ordinary start of that byte's kind, a dead (terminal)
    state for a dropped start, or a copy of the start that dies on a byte of G.  Returns the DFA and
    PRE's index; the states already there keep their numbers."""
    x, z, g = sets
    n, ncls = dfa.n_states, dfa.n_classes
    reps = [int(np.flatnonzero(dfa.cmap == c)[0]) for c in range(ncls)]
    for cs in (x, z, g):                         # the partition respects every CHAR set of the pattern
        for c in range(ncls):
            inside = [(cs >> int(b)) & 1 for b in np.flatnonzero(dfa.cmap == c)]
            assert min(inside) == max(inside)
    rows = [list(r) for r in dfa.trans.astype(np.int64)]
    flags = list(dfa.flags)
    dead = next((i for i in range(n) if flags[i] == 2 and all(t == i for t in rows[i])), -1)
    if dead < 0:
        dead = len(rows)
        rows.append([dead] * (ncls + 1))
        flags.append(2)
    die_g: Dict[int, int] = {}
    pre_row = []
    for c, r in enumerate(reps):
        start = dfa.start[_kind_of_byte(r)]
        if not (x >> r) & 1 or ((z >> r) & 1 and not g):
            pre_row.append(start)
        elif not (z >> r) & 1:
            pre_row.append(dead)
        else:
            if start not in die_g:
                die_g[start] = len(rows)
                rows.append([dead if c2 < ncls and (g >> reps[c2]) & 1 else t for c2, t in enumerate(rows[start])])
                flags.append(flags[start])
            pre_row.append(die_g[start])
    pre = len(rows)
    rows.append(pre_row + [dead])
    flags.append(0)
    if len(rows) > 65535:
        raise RuleError("DFA too large for 16-bit state ids")
    return DFA(dfa.cmap, np.array(rows, dtype=np.uint16), np.array(flags, dtype=np.uint8), dfa.start, []), pre


def minimize(dfa: DFA) -> DFA:
    """Moore partition refinement; initial blocks split by (flags, accept set)."""
    S = dfa.n_states
    if dfa.accept:
        sig0 = [(int(f), acc) for f, acc in zip(dfa.flags, dfa.accept)]
    else:
        sig0 = [(int(f),) for f in dfa.flags]
    uniq = {}
    block = np.array([uniq.setdefault(s, len(uniq)) for s in sig0], dtype=np.int64)
    nblocks = len(uniq)
    while True:
        sig = np.concatenate([block[:, None], block[dfa.trans]], axis=1)
        _, nb = np.unique(sig, axis=0, return_inverse=True)
        nb = nb.reshape(-1)
        n = int(nb.max()) + 1
        if n == nblocks:
            break
        block, nblocks = nb, n
    # renumber: keep start states first (stable), flagged states last (threshold test in kernels)
    rep = {}
    for s in range(S):
        rep.setdefault(int(block[s]), s)
    order = sorted(rep.keys(), key=lambda b: (1 if dfa.flags[rep[b]] else 0, rep[b]))
    newid = {b: i for i, b in enumerate(order)}
    trans = np.zeros((nblocks, dfa.trans.shape[1]), dtype=np.uint16)
    flags = np.zeros(nblocks, dtype=np.uint8)
    accept = [()] * nblocks if dfa.accept else []
    for b in order:
        s = rep[b]
        i = newid[b]
        trans[i] = [newid[int(block[t])] for t in dfa.trans[s]]
        flags[i] = dfa.flags[s]
        if dfa.accept:
            accept[i] = dfa.accept[s]
    start = [newid[int(block[s])] for s in dfa.start]
    if nblocks > 65535:
        raise RuleError("DFA too large for 16-bit state ids")
    return DFA(dfa.cmap, trans, flags, start, accept)


# ======================================================================= deidentify_config ====
# What happens to a finding's bytes (dlp_config.yaml:195-199): per info type, the first transformation
# that lists it, else the first without info_types, else the bytes stay (DLP leaves findings no
# transformation names).  The values are the engine's PII_XF_* (include/pii_engine.h).
XF_INFO_TYPE, XF_REPLACE, XF_REDACT, XF_MASK, XF_KEEP, XF_HASH, XF_FPE = range(7)
XF_MASK_WORDS = 8          # per type: char | reverse << 8, number_to_mask, 4 words of skip set, 2 spare
XF_REPLACE_MAX = 255
XF_HASH_LEN = 44           # base64 of a SHA-256 digest
XF_HASH_KEY_WORDS = 16     # per key: the inner, then the outer HMAC midstate (8 words each)
XF_FPE_KEY_WORDS = 64      # per key: Nr, the 4 * (Nr + 1) <= 60 AES round-key words, zeros
XF_FPE_ALPHA_WORDS = 68    # per alphabet: radix, nmin, nmax, 0; byte -> digit [128]; digit -> byte [96]; b(v) [32]
XF_FPE_NMAX = 64           # numerals the engine encrypts at most (v <= 32: b(v) has 32 entries)
XF_FPE_KEYS_MAX = 16       # distinct FPE keys in one config (the kernels hold the round keys in LDS)
_XF_PRIMITIVES = {"replace_with_info_type_config": XF_INFO_TYPE, "replace_config": XF_REPLACE,
                  "redact_config": XF_REDACT, "character_mask_config": XF_MASK, "crypto_hash_config": XF_HASH}
# every other primitive of DLP's PrimitiveTransformation: named in the error when one is configured
# (crypto_replace_ffx_fpe_config: refused only without fpe=True, see _parse_primitive)
_XF_UNSUPPORTED = ("crypto_replace_ffx_fpe_config", "crypto_deterministic_config",
                   "date_shift_config", "bucketing_config", "fixed_size_bucketing_config", "time_part_config",
                   "replace_dictionary_config")
_XF_COMMON = {"NUMERIC": "0123456789", "ALPHA_UPPER_CASE": "ABCDEFGHIJKLMNOPQRSTUVWXYZ",
              "ALPHA_LOWER_CASE": "abcdefghijklmnopqrstuvwxyz",
              "PUNCTUATION": "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~", "WHITESPACE": " \t\n\r\x0b\x0c"}


@dataclass
class Transform:
    kind: int
    value: bytes = b""         # XF_REPLACE: the replacement
    mask_char: int = 0x2A      # XF_MASK
    count: int = 0             # 0 = every character
    reverse: bool = False
    skip: int = 0              # 128-bit ASCII set: copied and not counted
    key: bytes = b""           # XF_HASH: the HMAC-SHA256 key (32 or 64 bytes); XF_FPE: the AES key (16, 24, 32)
    alphabet: str = ""         # XF_FPE: the numerals' characters, a numeral's value = its position


def _parse_mask(cfg: dict) -> Transform:
    cfg = cfg or {}
    unknown = set(cfg) - {"masking_character", "number_to_mask", "reverse_order", "characters_to_ignore"}
    if unknown:
        raise RuleError(f"character_mask_config: unsupported field {sorted(unknown)[0]}")
    ch = cfg.get("masking_character", "*")
    if not isinstance(ch, str) or len(ch) != 1 or ord(ch) > 127:
        raise RuleError(f"character_mask_config: masking_character {ch!r} is not one ASCII character")
    n = cfg.get("number_to_mask", 0) or 0
    if isinstance(n, bool) or not isinstance(n, int) or n < 0 or n >= 1 << 32:
        raise RuleError(f"character_mask_config: number_to_mask {n!r} is not a count >= 0")
    rev = cfg.get("reverse_order", False)
    if not isinstance(rev, bool):
        raise RuleError(f"character_mask_config: reverse_order {rev!r} is not true or false")
    skip = 0
    for ign in cfg.get("characters_to_ignore", []) or []:
        if set(ign) - {"characters_to_skip", "common_characters_to_ignore"} or len(ign) != 1:
            raise RuleError(f"character_mask_config: unsupported characters_to_ignore entry {ign!r}")
        if "characters_to_skip" in ign:
            chars = ign["characters_to_skip"]
            if not isinstance(chars, str) or any(ord(c) > 127 for c in chars):
                raise RuleError(f"character_mask_config: characters_to_skip {chars!r} is not ASCII")
        else:
            cls = ign["common_characters_to_ignore"]
            if cls not in _XF_COMMON:
                raise RuleError(f"character_mask_config: unknown common_characters_to_ignore {cls!r}")
            chars = _XF_COMMON[cls]
        for c in chars:
            skip |= 1 << ord(c)
    return Transform(XF_MASK, mask_char=ord(ch), count=n, reverse=rev, skip=skip)


# crypto_hash_config: a finding becomes base64(HMAC-SHA256(key, finding bytes)).  The key fills at most
# one 64-byte block, so HMAC's two keyed blocks (key ^ 0x36.., key ^ 0x5c..) can be compressed here, once:
# the blob carries the two chaining values (midstates) per key and the engine continues from them.
# hashlib does not expose a chaining value, hence the compression function below (FIPS 180-4, 6.2.2).
_SHA256_K = (
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2)
SHA256_IV = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)


def sha256_compress(state: Sequence[int], block: bytes) -> Tuple[int, ...]:
    """one SHA-256 compression: the chaining value after `block` (64 bytes) from chaining value `state`"""
    assert len(block) == 64 and len(state) == 8
    M = 0xFFFFFFFF

    def rotr(x, n):
        return ((x >> n) | (x << (32 - n))) & M
    w = list(struct.unpack(">16I", block))
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M)
    a, b, c, d, e, f, g, h = state
    for i in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & M & g)) + _SHA256_K[i] + w[i]) & M
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M
        a, b, c, d, e, f, g, h = (t1 + t2) & M, a, b, c, (d + t1) & M, e, f, g
    return tuple((x + y) & M for x, y in zip(state, (a, b, c, d, e, f, g, h)))


def hmac_midstates(key: bytes) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(inner, outer): the SHA-256 chaining values after key ^ 0x36.. and after key ^ 0x5c.. (key <= 64 bytes)"""
    assert len(key) <= 64
    k = key.ljust(64, b"\0")
    return (sha256_compress(SHA256_IV, bytes(b ^ 0x36 for b in k)),
            sha256_compress(SHA256_IV, bytes(b ^ 0x5C for b in k)))


def _parse_hash(cfg: dict) -> Transform:
    cfg = cfg or {}
    unknown = set(cfg) - {"crypto_key"}
    if unknown:
        raise RuleError(f"crypto_hash_config: unsupported field {sorted(unknown)[0]}")
    ck = cfg.get("crypto_key")
    if not isinstance(ck, dict) or not ck:
        raise RuleError("crypto_hash_config: crypto_key is missing")
    for k in ck:
        if k != "unwrapped":
            known = "unsupported" if k in ("transient", "kms_wrapped") else "unknown"
            raise RuleError(f"crypto_hash_config: {known} crypto_key form {k} (only unwrapped is supported)")
    uw = ck["unwrapped"]
    if not isinstance(uw, dict) or "key" not in uw:
        raise RuleError("crypto_hash_config: crypto_key.unwrapped.key is missing")
    unknown = set(uw) - {"key"}
    if unknown:
        raise RuleError(f"crypto_hash_config: unsupported field unwrapped.{sorted(unknown)[0]}")
    b64 = uw["key"]
    try:
        if not isinstance(b64, str):
            raise ValueError
        key = base64.b64decode(b64, validate=True)
    except ValueError:
        raise RuleError("crypto_hash_config: crypto_key.unwrapped.key is not base64") from None
    if len(key) not in (32, 64):
        raise RuleError(f"crypto_hash_config: crypto_key.unwrapped.key is {len(key)} bytes (not 32 or 64)")
    return Transform(XF_HASH, key=key)


# crypto_replace_ffx_fpe_config: a finding's characters of the alphabet are encrypted among themselves with
# FF1 (NIST SP 800-38G) over AES under an empty tweak; every other byte stays.  The blob carries
# the AES round keys (FIPS-197 5.2), expanded here, and per alphabet the two character maps, the limits on
# the numeral count and b(v), the byte length of radix^v - 1, which FF1 defines through a logarithm.
_FPE_NAME = "crypto_replace_ffx_fpe_config"
_FPE_COMMON = {"NUMERIC": "0123456789", "HEXADECIMAL": "0123456789ABCDEF",
               "UPPER_CASE_ALPHA_NUMERIC": "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ",
               "ALPHA_NUMERIC": "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"}


def _aes_sbox() -> List[int]:
    """FIPS-197 5.1.1: the multiplicative inverse in GF(2^8) (p runs through the powers of 3, q through
    their inverses), then the affine transformation"""
    box = [0x63] * 256
    p = q = 1
    while True:
        p = (p ^ (p << 1) ^ (0x1B if p & 0x80 else 0)) & 0xFF
        q ^= q << 1
        q ^= q << 2
        q ^= q << 4
        q &= 0xFF
        if q & 0x80:
            q ^= 0x09
        x = q
        for k in range(1, 5):
            x ^= ((q << k) | (q >> (8 - k))) & 0xFF
        box[p] = x ^ 0x63
        if p == 1:
            return box


_AES_SBOX = _aes_sbox()


def aes_round_keys(key: bytes) -> Tuple[int, ...]:
    """the key schedule w[0 .. 4 * (Nr + 1)) of a 16-, 24- or 32-byte key, big-endian words"""
    assert len(key) in (16, 24, 32)
    nk = len(key) // 4
    w = list(struct.unpack(f">{nk}I", key))

    def sub(x):
        return int.from_bytes(bytes(_AES_SBOX[b] for b in x.to_bytes(4, "big")), "big")
    rcon = 1
    for i in range(nk, 4 * (nk + 7)):
        t = w[-1]
        if i % nk == 0:
            t = sub(((t << 8) | (t >> 24)) & 0xFFFFFFFF) ^ (rcon << 24)
            rcon = (rcon << 1) ^ (0x11B if rcon & 0x80 else 0)
        elif nk == 8 and i % nk == 4:
            t = sub(t)
        w.append(w[i - nk] ^ t)
    return tuple(w)


def fpe_key_words(key: bytes) -> np.ndarray:
    """one xf.fpe_key record (XF_FPE_KEY_WORDS words): Nr, the round keys, zeros"""
    w = aes_round_keys(key)
    rec = np.zeros(XF_FPE_KEY_WORDS, dtype=np.uint32)
    rec[0] = len(w) // 4 - 1
    rec[1:1 + len(w)] = w
    return rec


def fpe_limits(radix: int) -> Tuple[int, int]:
    """(nmin, nmax) numerals: the least n >= 2 with radix^n >= 100 (SP 800-38G); min(2 * vmax, XF_FPE_NMAX)
    with radix^vmax <= 2^128, so that NUM(B) fits 16 bytes"""
    nmin = 2
    while radix ** nmin < 100:
        nmin += 1
    vmax = 1
    while radix ** (vmax + 1) <= 1 << 128:
        vmax += 1
    return nmin, min(2 * vmax, XF_FPE_NMAX)


def fpe_alphabet_words(alphabet: str) -> np.ndarray:
    """one xf.fpe_alpha record (XF_FPE_ALPHA_WORDS words)"""
    radix = len(alphabet)
    nmin, nmax = fpe_limits(radix)
    to_digit = np.full(128, 0xFF, dtype=np.uint8)
    to_byte = np.zeros(96, dtype=np.uint8)
    for d, ch in enumerate(alphabet):
        to_digit[ord(ch)] = d
        to_byte[d] = ord(ch)
    # b(v), v = 1 .. 32: the bytes of radix^v - 1; past nmax / 2 it is not used (16 there, so the row stays monotonous)
    bv = np.array([min(((radix ** v - 1).bit_length() + 7) // 8, 16) for v in range(1, 33)], dtype=np.uint8)
    rec = np.concatenate([np.array([radix, nmin, nmax, 0], dtype="<u4").view(np.uint8), to_digit, to_byte, bv])
    assert rec.size == 4 * XF_FPE_ALPHA_WORDS
    return rec.view("<u4").astype(np.uint32)


def _parse_fpe(cfg: dict) -> Transform:
    cfg = cfg or {}
    fields = {"crypto_key", "common_alphabet", "custom_alphabet"}
    for k in ("context", "radix", "surrogate_info_type"):
        if k in cfg:
            raise RuleError(f"{_FPE_NAME}: {k} is not supported")
    unknown = set(cfg) - fields
    if unknown:
        raise RuleError(f"{_FPE_NAME}: unsupported field {sorted(unknown)[0]}")
    ck = cfg.get("crypto_key")
    if not isinstance(ck, dict) or not ck:
        raise RuleError(f"{_FPE_NAME}: crypto_key is missing")
    for k in ck:
        if k != "unwrapped":
            known = "unsupported" if k in ("transient", "kms_wrapped") else "unknown"
            raise RuleError(f"{_FPE_NAME}: {known} crypto_key form {k} (only unwrapped is supported)")
    uw = ck["unwrapped"]
    if not isinstance(uw, dict) or "key" not in uw:
        raise RuleError(f"{_FPE_NAME}: crypto_key.unwrapped.key is missing")
    unknown = set(uw) - {"key"}
    if unknown:
        raise RuleError(f"{_FPE_NAME}: unsupported field unwrapped.{sorted(unknown)[0]}")
    try:
        if not isinstance(uw["key"], str):
            raise ValueError
        key = base64.b64decode(uw["key"], validate=True)
    except ValueError:
        raise RuleError(f"{_FPE_NAME}: crypto_key.unwrapped.key is not base64") from None
    if len(key) not in (16, 24, 32):
        raise RuleError(f"{_FPE_NAME}: crypto_key.unwrapped.key is {len(key)} bytes (not 16, 24 or 32)")
    if ("common_alphabet" in cfg) == ("custom_alphabet" in cfg):
        raise RuleError(f"{_FPE_NAME}: exactly one of common_alphabet and custom_alphabet is needed")
    if "common_alphabet" in cfg:
        name = cfg["common_alphabet"]
        if not isinstance(name, str) or name not in _FPE_COMMON:
            raise RuleError(f"{_FPE_NAME}: unknown common_alphabet {name!r}")
        alphabet = _FPE_COMMON[name]
    else:
        alphabet = cfg["custom_alphabet"]
        if not isinstance(alphabet, str) or not 2 <= len(alphabet) <= 95:
            raise RuleError(f"{_FPE_NAME}: custom_alphabet does not hold 2 to 95 characters")
        for ch in alphabet:
            if not 0x20 <= ord(ch) <= 0x7E:
                raise RuleError(f"{_FPE_NAME}: custom_alphabet character {ch!r} is not printable ASCII")
        if len(set(alphabet)) != len(alphabet):
            raise RuleError(f"{_FPE_NAME}: custom_alphabet repeats a character")
    return Transform(XF_FPE, key=key, alphabet=alphabet)


def _parse_primitive(prim: dict, fpe: bool = False) -> Transform:
    prim = prim or {}
    if len(prim) != 1:
        raise RuleError(f"a primitive_transformation holds exactly one primitive, not {sorted(prim)}")
    (name, cfg), = prim.items()
    if fpe and name == _FPE_NAME:
        return _parse_fpe(cfg)
    if name not in _XF_PRIMITIVES:
        known = "unsupported" if name in _XF_UNSUPPORTED else "unknown"
        raise RuleError(f"{known} primitive transformation {name}")
    kind = _XF_PRIMITIVES[name]
    if kind == XF_MASK:
        return _parse_mask(cfg)
    if kind == XF_HASH:
        return _parse_hash(cfg)
    if kind == XF_REPLACE:
        nv = (cfg or {}).get("new_value", {}) or {}
        if set(nv) != {"string_value"} or not isinstance(nv["string_value"], str):
            raise RuleError("replace_config: only new_value.string_value is supported")
        value = nv["string_value"].encode("utf-8")
        if len(value) > XF_REPLACE_MAX:
            raise RuleError(f"replace_config: string_value is {len(value)} bytes (more than {XF_REPLACE_MAX})")
        return Transform(XF_REPLACE, value=value)
    if cfg:
        raise RuleError(f"{name}: unsupported field {sorted(cfg)[0]}")
    return Transform(kind)


def parse_deidentify(dlp_config: dict, type_names: Sequence[str], fpe: bool = False) -> List[Transform]:
    """deidentify_config -> one Transform per info type (type order).  No block: "[TYPE]" for all.
    fpe: accept crypto_replace_ffx_fpe_config (_parse_fpe).  Without it the primitive is refused as
    unsupported, as it always was; compile_default asks for it."""
    if "deidentify_config" not in dlp_config or dlp_config["deidentify_config"] is None:
        return [Transform(XF_INFO_TYPE) for _ in type_names]
    de = dlp_config["deidentify_config"]
    for k in de:
        if k != "info_type_transformations":
            raise RuleError(f"deidentify_config: {k} is not supported")
    itt = de.get("info_type_transformations", {}) or {}
    for k in itt:
        if k != "transformations":
            raise RuleError(f"info_type_transformations: {k} is not supported")
    known = set(type_names)
    listed: Dict[str, Transform] = {}
    catch_all: Optional[Transform] = None
    for entry in itt.get("transformations", []) or []:
        for k in entry:
            if k not in ("info_types", "primitive_transformation"):
                raise RuleError(f"transformation: {k} is not supported")
        if "primitive_transformation" not in entry:
            raise RuleError("transformation without a primitive_transformation")
        tf = _parse_primitive(entry["primitive_transformation"], fpe)
        names = [it.get("name") for it in entry.get("info_types", []) or []]
        for n in names:
            if n not in known:
                raise RuleError(f"deidentify_config names an unknown info type {n}")
            listed.setdefault(n, tf)
        if not names and catch_all is None:
            catch_all = tf
    default = catch_all if catch_all is not None else Transform(XF_KEEP)
    return [listed.get(n, default) for n in type_names]


def transform_sections(transforms: Sequence[Transform]) -> "OrderedDict[str, np.ndarray]":
    """The optional xf.* blob sections; none when every type keeps the "[TYPE]" token (the engine's
    behaviour without them), so such a config compiles to the blob it always did."""
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    if all(t.kind == XF_INFO_TYPE for t in transforms):
        return out
    T = len(transforms)
    off = np.zeros(T + 1, dtype=np.uint32)
    repl = b""
    mask = np.zeros((T, XF_MASK_WORDS), dtype=np.uint32)
    for i, t in enumerate(transforms):
        if t.kind == XF_REPLACE:
            repl += t.value
        if t.kind == XF_HASH:              # a placeholder of the surrogate's length; k_hash writes the bytes
            repl += b"=" * XF_HASH_LEN
        off[i + 1] = len(repl)
        if t.kind == XF_MASK:
            mask[i, 0] = t.mask_char | (0x100 if t.reverse else 0)
            mask[i, 1] = t.count
            for w in range(4):
                mask[i, 2 + w] = (t.skip >> (32 * w)) & 0xFFFFFFFF
    out["xf.kind"] = np.array([t.kind for t in transforms], dtype=np.uint8)
    out["xf.repl_off"] = off
    out["xf.repl"] = np.frombuffer(repl or b"\0", dtype=np.uint8).copy()
    out["xf.mask"] = mask.reshape(-1)
    # crypto_hash_config (only with a hash type): per type a key index, per distinct key its two midstates.
    # The midstates are as secret as the key: whoever holds them computes the same surrogates.
    if any(t.kind == XF_HASH for t in transforms):
        keys: List[bytes] = []
        for t in transforms:
            if t.kind == XF_HASH and t.key not in keys:
                keys.append(t.key)
        out["xf.hash_key"] = np.array([keys.index(t.key) if t.kind == XF_HASH else 0 for t in transforms],
                                      dtype=np.uint32)
        out["xf.hash_mid"] = np.array([w for k in keys for mid in hmac_midstates(k) for w in mid], dtype=np.uint32)
    # crypto_replace_ffx_fpe_config (only with an FPE type): per type key index | alphabet index << 16, per
    # distinct key its AES round keys, per distinct alphabet its record.  The round keys are as secret as the
    # key, like the midstates: the raw key follows from them.
    if any(t.kind == XF_FPE for t in transforms):
        fkeys: List[bytes] = []
        alphas: List[str] = []
        for t in transforms:
            if t.kind == XF_FPE and t.key not in fkeys:
                fkeys.append(t.key)
            if t.kind == XF_FPE and t.alphabet not in alphas:
                alphas.append(t.alphabet)
        if len(fkeys) > XF_FPE_KEYS_MAX:
            raise RuleError(f"{_FPE_NAME}: more than {XF_FPE_KEYS_MAX} distinct keys")
        out["xf.fpe"] = np.array([fkeys.index(t.key) | alphas.index(t.alphabet) << 16 if t.kind == XF_FPE else 0
                                  for t in transforms], dtype=np.uint32)
        out["xf.fpe_key"] = np.concatenate([fpe_key_words(k) for k in fkeys])
        out["xf.fpe_alpha"] = np.concatenate([fpe_alphabet_words(a) for a in alphas])
    return out


# ================================================================================ rule model ====
@dataclass
class Pattern:
    pid: int
    type_name: str
    pattern: str
    likelihood: int
    validator: Optional[str]
    custom: bool
    scan_prefix: Optional[int] = None     # characters the SCAN prefilter keeps (None: SCAN_BUDGET)


@dataclass
class HotRule:
    pattern: str
    window_before: int
    window_after: int
    fixed: int               # 0 = use relative
    relative: int


class Rules:
    """The rule model both the engine blob and the docs are generated from."""

    def __init__(self, dlp_config: dict, builtin: dict, fpe: bool = False):
        insp = dlp_config.get("inspect_config", {}) or {}
        self.raw = dlp_config
        self.base_info_types = [it.get("name") for it in insp.get("info_types", [])]
        self.custom_defs = list(insp.get("custom_info_types", []) or [])
        self.custom_names = [c.get("info_type", {}).get("name") for c in self.custom_defs]
        self.context_keywords: "OrderedDict[str, list]" = OrderedDict(dlp_config.get("context_keywords", {}) or {})
        dets = builtin["detectors"]
        order = []
        for n in self.base_info_types + self.custom_names + list(dets.keys()) + list(self.context_keywords):
            if n not in order:
                order.append(n)
        # types of external detectors (the NER): last in the type order, no pattern, no variant
        self.external_types = [n for n in (builtin.get("external_types") or []) if n not in order]
        order += self.external_types
        self.type_names = order
        self.type_id = {n: i for i, n in enumerate(order)}
        self.patterns: List[Pattern] = []
        for name, variants in dets.items():
            if name in self.custom_names:
                continue
            for v in variants:
                self.patterns.append(Pattern(len(self.patterns), name, v["pattern"],
                                             lik_value(v.get("likelihood", "POSSIBLE")), v.get("validator"), False,
                                             v.get("scan_prefix")))
        for c in self.custom_defs:
            name = c["info_type"]["name"]
            if "regex" in c:
                pat = c["regex"]["pattern"]
            elif "dictionary" in c:
                words = c["dictionary"]["word_list"]["words"]
                pat = r"(?i)\b(?:" + "|".join(re.escape(w) for w in words) + r")\b"
            else:
                raise RuleError(f"unsupported custom infoType {name}")
            # dictionary words: a 3-character prefix fires at most word starts of ordinary text (13x the
            # matches on config 5's text), a 4-character one about 1.5x (SCAN prefilter, see plan_scan_groups)
            self.patterns.append(Pattern(len(self.patterns), name, pat,
                                         lik_value(c.get("likelihood", "VERY_LIKELY")), None, True,
                                         DICT_SCAN_PREFIX if "dictionary" in c else None))
        for p in self.patterns:
            if p.validator not in VALIDATOR_IDS:
                raise RuleError(f"unknown validator {p.validator}")
        # context keyword groups (main.py:558-578): group g -> (type, regex or None, always-hit)
        self.kw_groups = []
        for t, kws in self.context_keywords.items():
            # the keywords as extract_expected_pii compares them: UTF-8 bytes against the ASCII-lowered text
            # (SURVEY A.8), so the pattern is a bytes pattern -- (?i) folds A-Z alone, and "café" is four
            # literal bytes after "caf" that "CAFÉ" does not hold
            kws = [str(k).encode("utf-8") for k in (kws or [])]
            always = any(k == b"" for k in kws)
            # a keyword with a byte of A-Z never hits the lowered text
            usable = [k for k in kws if k and not any(65 <= c <= 90 for c in k)]
            pat = b"(?i)(?:" + b"|".join(re.escape(k) for k in usable) + b")" if usable else None
            self.kw_groups.append((t, pat, always))
        # Every other info type becomes a keyword-less context group, so that a context record naming
        # it (call_dlp_for_redaction(transcript, {"expected_pii_type": t}), main.py:614-686) has a
        # compiled variant.  extract_expected_pii never returns one (no keywords).  Large rule sets
        # (config 5) skip this: V * T variant tables would not fit the kernels' LDS images.
        self.n_keyword_groups = len(self.kw_groups)
        if len(self.type_names) <= PSEUDO_GROUP_MAX_TYPES:
            named = {t for t, _, _ in self.kw_groups} | set(self.external_types)
            self.kw_groups.extend((t, None, False) for t in self.type_names if t not in named)

        self.transforms = parse_deidentify(dlp_config, self.type_names, fpe)

    @classmethod
    def load(cls, dlp_config_path: Optional[str] = None, builtin_path: Optional[str] = None,
             fpe: bool = False) -> "Rules":
        dlp_config_path = dlp_config_path or os.path.join(RULES_DIR, "dlp_config.json")
        builtin_path = builtin_path or os.path.join(RULES_DIR, "builtin_infotypes.yaml")
        with open(dlp_config_path) as f:
            cfg = json.load(f) if dlp_config_path.endswith(".json") else yaml.safe_load(f)
        with open(builtin_path) as f:
            builtin = yaml.safe_load(f)
        return cls(cfg, builtin, fpe)

    # ---- a6, main.py:609-686, restated statelessly -------------------------------
    def merged_inspect_config(self, expected_type: Optional[str]) -> dict:
        import copy
        cfg = copy.deepcopy(self.raw.get("inspect_config", {}) or {})
        if not expected_type:
            return cfg
        custom = next((c for c in self.custom_defs if c.get("info_type", {}).get("name") == expected_type), None)
        if custom is not None:
            cfg.setdefault("custom_info_types", [])
            if expected_type not in {c.get("info_type", {}).get("name") for c in cfg["custom_info_types"]}:
                cfg["custom_info_types"].append(copy.deepcopy(custom))
            return cfg
        cfg.setdefault("info_types", [])
        if expected_type not in {it.get("name") for it in cfg["info_types"]}:
            cfg["info_types"].append({"name": expected_type})
        cfg.setdefault("rule_set", [])
        found = False
        for entry in cfg["rule_set"]:
            if "info_types" in entry and expected_type in {it.get("name") for it in entry["info_types"]}:
                for rule in entry.get("rules", []):
                    if "hotword_rule" in rule and "likelihood_adjustment" in rule["hotword_rule"]:
                        rule["hotword_rule"]["likelihood_adjustment"]["fixed_likelihood"] = VERY_LIKELY
                        found = True
                        break
                if found:
                    break
        if not found:
            cfg["rule_set"].append({"info_types": [{"name": expected_type}], "rules": [{"hotword_rule": {
                "hotword_regex": {"pattern": ".+"}, "proximity": {"window_before": 100, "window_after": 100},
                "likelihood_adjustment": {"fixed_likelihood": VERY_LIKELY}}}]})
        return cfg

    def variants(self):
        """Variant 0 = no context; variant 1+g = expected type of keyword group g."""
        out = [self.merged_inspect_config(None)]
        for t, _, _ in self.kw_groups:
            out.append(self.merged_inspect_config(t))
        return out


# =================================================================================== blob =======
_DT = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.uint32): 3, np.dtype(np.int32): 4,
       np.dtype(np.int64): 5, np.dtype(np.int8): 6}


def _sections_to_blob(sections: "OrderedDict[str, np.ndarray]") -> bytes:
    out = io.BytesIO()
    out.write(BLOB_MAGIC)
    out.write(struct.pack("<I", len(sections)))
    for name, arr in sections.items():
        arr = np.ascontiguousarray(arr)
        nb = name.encode()
        out.write(struct.pack("<I", len(nb)))
        out.write(nb)
        out.write(struct.pack("<IQ", _DT[arr.dtype], arr.nbytes))
        out.write(arr.tobytes())
        pad = (-out.tell()) % 8
        out.write(b"\0" * pad)
    return out.getvalue()


def blob_sections(blob: bytes) -> "OrderedDict[str, np.ndarray]":
    inv = {v: k for k, v in _DT.items()}
    assert blob[:8] == BLOB_MAGIC
    (n,) = struct.unpack_from("<I", blob, 8)
    off = 12
    out = OrderedDict()
    for _ in range(n):
        (ln,) = struct.unpack_from("<I", blob, off)
        off += 4
        name = blob[off:off + ln].decode()
        off += ln
        dt, nbytes = struct.unpack_from("<IQ", blob, off)
        off += 12
        out[name] = np.frombuffer(blob, dtype=inv[dt], count=nbytes // inv[dt].itemsize, offset=off).copy()
        off += nbytes
        off += (-off) % 8
    return out


@dataclass
class Compiled:
    rules: Rules
    scan_d: MealyDFA          # reverse relaxed detector prefilter
    scan_k: MealyDFA          # reverse exact context-keyword groups
    first: List[DFA]
    hot: List[DFA]
    hot_rules: List[HotRule]
    sections: "OrderedDict[str, np.ndarray]"
    blob: bytes
    scan_groups: List[List[int]] = None     # pattern ids of each SCAN group (group 0 first)


SCAN_BUDGET = 3     # prefix characters per detector pattern in the SCAN prefilter


def _acc_tables(m: MealyDFA):
    """acc_off/acc_ids flattening of a Mealy DFA's accept sets (index 0 = empty)."""
    off = np.zeros(len(m.acc_sets) + 1, dtype=np.uint32)
    ids: List[int] = []
    for i, s in enumerate(m.acc_sets):
        ids.extend(s)
        off[i + 1] = len(ids)
    return off, np.array(ids or [0], dtype=np.uint16)


SCAN_LDS_BYTES = 65536          # k_scan tables: u16 LDS byte addresses (class map + D rows + K rows)
SCAN_CMAP_BYTES = 1024
SCAN_GROUP_BYTES = 62 * 1024    # D table of a scan group >= 1 that keeps 16-bit byte addresses (two
                                # k_scan workgroups per CU); its K is a 1-row never-accepting stub
SCAN_WIDE_BYTES = 124 * 1024    # a WIDE group >= 1 (engine: rows padded to 4 entries, entries = offset / 2,
                                # one workgroup per CU): up to 64k transitions
SPILL_PREFIX = 10               # prefix of the built-ins moved out of group 0 (plan_scan_groups)
SCAN_GROUPS_MAX = 8             # k_pairs_merge merges at most this many per-group event lists per lane
# Exclusion rules (mirrors of csrc/pii_layout.h).  A rule set whose exclusions k_select can decide while it
# streams a lane (FULL_MATCH only, at most NE_MAX excluder patterns, no type both excluded and excluding)
# compiles to var.excl_* / det.exidx; any other is GENERAL: those stay empty and k_exclude reads var.xg_* /
# det.xgidx instead.
NE_MAX = 2                      # excluder patterns of the streaming form
NX_MAX = 64                     # excluder patterns of a general rule set
XG_PARTIAL = 0x8000             # var.xg_ids entry: excluder type id | this bit for MATCHING_TYPE_PARTIAL_MATCH
MATCHING_TYPES = ("MATCHING_TYPE_FULL_MATCH", "MATCHING_TYPE_PARTIAL_MATCH")
DICT_SCAN_PREFIX = 4            # SCAN prefix of dictionary infoTypes (Rules)
# Exclusion rules that test the candidate's own text (exclusion_rule.regex / .dictionary, by matching
# type) or the text around it (exclusion_rule.exclude_by_hotword): k_excl_text runs the rule's HOT-form
# automaton over the quote or the proximity windows.  xt.rule entry = (kind, window_before, window_after, 0).
XT_SEARCH, XT_FULL, XT_INVERSE, XT_HOTWORD = range(4)
XT_FORMS = ("exclude_info_types", "regex", "dictionary", "exclude_by_hotword")
XT_KIND = {"MATCHING_TYPE_FULL_MATCH": XT_FULL, "MATCHING_TYPE_PARTIAL_MATCH": XT_SEARCH,
           "MATCHING_TYPE_INVERSE_MATCH": XT_INVERSE}


@dataclass(frozen=True)
class TextExcl:
    """one text exclusion rule: `pattern` is searched in the quote (XT_SEARCH), must match all of it
    (XT_FULL: drop, XT_INVERSE: keep), or is searched in the proximity windows (XT_HOTWORD)"""
    kind: int
    pattern: str
    window_before: int = 0
    window_after: int = 0


def parse_text_exclusion(ex: dict) -> TextExcl:
    """exclusion_rule.regex / .dictionary / .exclude_by_hotword -> TextExcl, or the RuleError naming the
    field that is not supported"""
    mt = ex.get("matching_type", "MATCHING_TYPE_FULL_MATCH")
    if mt not in XT_KIND:
        raise RuleError(f"exclusion_rule: unknown matching_type {mt}")
    if "regex" in ex:
        rx = ex["regex"] or {}
        if rx.get("group_indexes"):
            raise RuleError("exclusion_rule.regex.group_indexes is not supported")
        if not isinstance(rx.get("pattern"), str):
            raise RuleError("exclusion_rule.regex without a pattern")
        return TextExcl(XT_KIND[mt], rx["pattern"])
    if "dictionary" in ex:
        dc = ex["dictionary"] or {}
        if "cloud_storage_path" in dc:
            raise RuleError("exclusion_rule.dictionary.cloud_storage_path is not supported (use word_list)")
        words = [str(w) for w in ((dc.get("word_list") or {}).get("words") or [])]
        if not words or any(not w for w in words):
            raise RuleError("exclusion_rule.dictionary.word_list.words is empty")
        for w in words:
            if not w.isascii():
                raise RuleError(f"exclusion_rule.dictionary.word_list.words: {w!r} is not ASCII")
        return TextExcl(XT_KIND[mt], r"(?i)\b(?:" + "|".join(re.escape(w) for w in words) + r")\b")
    hw = ex["exclude_by_hotword"] or {}
    rx = hw.get("hotword_regex") or {}
    if rx.get("group_indexes"):
        raise RuleError("exclusion_rule.exclude_by_hotword.hotword_regex.group_indexes is not supported")
    if not isinstance(rx.get("pattern"), str):
        raise RuleError("exclusion_rule.exclude_by_hotword without a hotword_regex.pattern")
    prox = hw.get("proximity") or {}
    wb, wa = int(prox.get("window_before", 0) or 0), int(prox.get("window_after", 0) or 0)
    if wb < 0 or wa < 0 or (wb == 0 and wa == 0):
        raise RuleError("exclusion_rule.exclude_by_hotword.proximity has no window_before / window_after")
    return TextExcl(XT_HOTWORD, rx["pattern"], wb, wa)


def _table_bytes(m: MealyDFA) -> int:
    return m.n_states * ((m.n_classes + 2) & ~1) * 2


def _table_bytes_wide(m: MealyDFA) -> int:
    return m.n_states * ((m.n_classes + 4) & ~3) * 2


def _scan_dfa(patterns: Sequence[Pattern], budget: int, max_bytes: Optional[int] = None,
              prefixes: bool = True) -> Optional[MealyDFA]:
    """prefixes: honour the detectors' scan_prefix (longer relaxed prefixes: fewer candidate pairs,
    more states); without, every pattern keeps `budget` characters."""
    nd = NFA()
    sd = [add_relaxed(nd, p.pattern, p.pid, (p.scan_prefix if prefixes else None) or budget, reverse=True)
          for p in patterns]
    try:
        m = build_mealy_dfa(nd, sd, max_bytes=max_bytes)
    except RuleError:
        if max_bytes is None:
            raise
        return None
    return m if max_bytes is None or _table_bytes(m) <= max_bytes else None


def _scan_dfa_fit(patterns: Sequence[Pattern], budget: int, max_bytes: int) -> Optional[MealyDFA]:
    """the automaton with the declared scan prefixes, else (too large) with `budget` for every pattern"""
    m = _scan_dfa(patterns, budget, max_bytes)
    if m is None and any(p.scan_prefix for p in patterns):
        m = _scan_dfa(patterns, budget, max_bytes, prefixes=False)
    return m


def _prefix_key(p: Pattern) -> str:
    return re.sub(r"^\(\?i\)|\\b", "", p.pattern).lower()


def plan_scan_groups(rules: Rules, budget: int, k_bytes: int) -> List[Tuple[List[Pattern], MealyDFA]]:
    """Split the detector patterns over reverse D automata that each fit k_scan's LDS (config 5: 500+
    custom types).  One automaton per independent pattern set multiplies the states (a product of
    the sets' tries), so large rule sets get several smaller automata, each stepped by its own
    k_scan pass.  Group 0 is stepped together with the keyword automaton K and holds every built-in
    and excluder pattern; the rest, ordered by prefix so that similar prefixes share states, is cut
    in halves until each half fits."""
    limit0 = SCAN_LDS_BYTES - SCAN_CMAP_BYTES - k_bytes
    whole = _scan_dfa_fit(rules.patterns, budget, limit0) if len(rules.patterns) <= 256 else None
    if whole is not None:
        return [(list(rules.patterns), whole)]
    excl = set()
    for insp in rules.variants():
        for rs in insp.get("rule_set", []) or []:
            for rule in rs.get("rules", []):
                if "exclusion_rule" in rule:
                    excl |= {it["name"] for it in rule["exclusion_rule"].get("exclude_info_types", {}).get(
                        "info_types", [])}
    base = [p for p in rules.patterns if not p.custom or p.type_name in excl]
    rest = sorted((p for p in rules.patterns if p.custom and p.type_name not in excl), key=_prefix_key)
    # group 0 keeps the declared prefixes: when they do not fit beside K (config 5's larger keyword
    # automaton), the non-excluder built-ins with the longest declared prefixes move to a group of their
    # own (one more k_scan pass) rather than every built-in falling back to `budget` characters --
    # short digit-run prefixes fire at every digit run of the custom types' ids
    spill: List[Pattern] = []
    g0 = _scan_dfa(base, budget, limit0)
    if g0 is None:
        spill = [p for p in base if p.type_name not in excl and p.scan_prefix]
        base = [p for p in base if not (p.type_name not in excl and p.scan_prefix)]
        g0 = _scan_dfa(base, budget, limit0) if base else None
    if g0 is None:
        spill, base = [], spill + base
        base.sort(key=lambda p: p.pid)
        g0 = _scan_dfa_fit(base, budget, limit0)
    if g0 is None:
        raise RuleError("the built-in detectors' SCAN automaton does not fit k_scan's LDS")
    out = [(base, g0)]

    def fits(m, wide):
        return m is not None and (_table_bytes(m) <= SCAN_GROUP_BYTES or
                                  (wide and _table_bytes_wide(m) <= SCAN_WIDE_BYTES and
                                   m.n_states * ((m.n_classes + 4) & ~3) <= 65536))

    def split(pats):
        # the declared prefixes (dictionary types: DICT_SCAN_PREFIX) are worth a split -- they cut the
        # candidate pairs several-fold -- so a set is halved before its prefixes are shortened.  A set
        # whose automaton fits a WIDE table stays one group (one k_scan workgroup per CU: 352 us per
        # pass at config 5 against 283 for a narrow pass, so one wide pass beats two narrow ones); only
        # a set too large for that is halved.  A single pattern whose automaton does not fit falls back
        # to `budget` characters.
        m = _scan_dfa(pats, budget, SCAN_WIDE_BYTES)
        if fits(m, True):
            out.append((pats, m))
            return
        if len(pats) == 1:
            m = _scan_dfa(pats, budget, SCAN_WIDE_BYTES, prefixes=False)
            if not fits(m, True):
                raise RuleError(f"the SCAN automaton of {pats[0].type_name} alone does not fit k_scan's LDS")
            out.append((pats, m))
            return
        h = len(pats) // 2
        split(pats[:h])
        split(pats[h:])
    if spill:
        # the spilled built-ins have a table of their own: their prefixes may grow to SPILL_PREFIX
        # (digit-run detectors: a 7-digit prefix still fires at every 7-9 digit custom id)
        long = [dataclasses.replace(p, scan_prefix=max(p.scan_prefix, SPILL_PREFIX)) for p in spill]
        m = _scan_dfa(long, budget, SCAN_GROUP_BYTES)
        if m is not None:
            out.append((sorted(long, key=lambda p: p.pid), m))
        else:
            split(sorted(spill, key=lambda p: p.pid))
    if rest:
        split(rest)
    if len(out) > SCAN_GROUPS_MAX:
        raise RuleError(f"{len(out)} SCAN groups (more than {SCAN_GROUPS_MAX})")
    return out


def compile_rules(rules: Rules, scan_budget: int = SCAN_BUDGET, text_exclusions: bool = False) -> Compiled:
    """text_exclusions: compile exclusion_rule.regex / .dictionary / .exclude_by_hotword (parse_text_exclusion).
    Off, the call keeps the contract it always had -- those forms are a RuleError naming the form -- so a
    caller that has not asked for them never gets a general rule set it did not expect; compile_default,
    the entry point of the service and the tools, asks for them."""
    P = len(rules.patterns)
    G = len(rules.kw_groups)
    if P == 0:
        raise RuleError("no detectors")
    # ---- SCAN (two Mealy automata stepped together, right to left) ----
    nk = NFA()
    sk = [add_relaxed(nk, pat, g, 0, reverse=True) for g, (_t, pat, _a) in enumerate(rules.kw_groups) if pat]
    if not sk:                       # no keywords: a one-state automaton that never accepts
        sk = [add_relaxed(nk, "\\xff\\x00\\xff", 0, 0, reverse=True)]
    scan_k = build_mealy_dfa(nk, sk)
    groups = plan_scan_groups(rules, scan_budget, _table_bytes(scan_k))
    scan_d = groups[0][1]
    for _, m in groups:
        if m.n_classes + 1 > 255:
            raise RuleError("too many byte classes")
    if scan_k.n_classes + 1 > 255:
        raise RuleError("too many byte classes")
    cmap2 = scan_d.cmap.astype(np.uint16) | (scan_k.cmap.astype(np.uint16) << 8)
    k_off, k_ids = _acc_tables(scan_k)

    # ---- FIRST: one anchored leftmost-first DFA per detector pattern ----
    first = []
    min_len = 1 << 30
    # window_ok: no detector can consume '\n' or test a text edge (\A, \Z).  Then no match crosses
    # the "\n" that joins a re-scan window, and a match inside one utterance is the same
    # match inside the window, which is what lets the engine re-scan windows incrementally.
    window_ok = 1
    # first_pre: per pattern, the PRE state of add_first_drop (absorbed match starts), -1 = none
    first_pre = np.full(P, -1, dtype=np.int32)
    for p in rules.patterns:
        n2 = NFA()
        st = add_pattern(n2, p.pattern, p.pid, reverse=False)
        d = build_first_dfa(n2, st)
        sets = first_drop_sets(p.pattern)
        if sets is not None:
            d, first_pre[p.pid] = add_first_drop(d, sets)
        first.append(d)
        min_len = min(min_len, _min_len(parse(p.pattern)))
        for k, b, cs in zip(n2.kind, n2.b, n2.cs):
            if (k == CHAR and cs & NEWLINE) or (k == ASSERT and b in (A_BEGIN, A_END)):
                window_ok = 0

    # ---- variants (context merge, main.py:609-686) + HOT rule DFAs ----
    T = len(rules.type_names)
    V = 1 + G
    hot_rules: List[HotRule] = []
    hot_index: Dict[tuple, int] = {}
    var_enabled = np.zeros((V, T), dtype=np.uint8)
    var_minlik = np.zeros(V, dtype=np.uint8)
    rule_off = np.zeros(V * T + 1, dtype=np.uint32)
    rule_ids: List[int] = []
    excl_off = np.zeros(V * T + 1, dtype=np.uint32)
    excl_ids: List[int] = []
    xt_rules: List[TextExcl] = []
    xt_index: Dict[TextExcl, int] = {}
    xt_off = np.zeros(V * T + 1, dtype=np.uint32)
    xt_ids: List[int] = []
    for v, insp in enumerate(rules.variants()):
        enabled = {it.get("name") for it in insp.get("info_types", [])}
        enabled |= {c.get("info_type", {}).get("name") for c in insp.get("custom_info_types", []) or []}
        for name in list(enabled) + rules.external_types:
            if name in rules.type_id:
                var_enabled[v, rules.type_id[name]] = 1
        var_minlik[v] = lik_value(insp.get("min_likelihood", DEFAULT_MIN_LIKELIHOOD))
        per_type_rules = [[] for _ in range(T)]
        per_type_excl = [[] for _ in range(T)]
        per_type_xt = [[] for _ in range(T)]
        for rs in insp.get("rule_set", []) or []:
            tnames = [it.get("name") for it in rs.get("info_types", [])]
            for rule in rs.get("rules", []):
                if "hotword_rule" in rule:
                    h = rule["hotword_rule"]
                    adj = h.get("likelihood_adjustment", {})
                    prox = h.get("proximity", {})
                    fixed = adj.get("fixed_likelihood")
                    hr = HotRule(h["hotword_regex"]["pattern"], int(prox.get("window_before", 0)),
                                 int(prox.get("window_after", 0)), 0 if fixed is None else lik_value(fixed),
                                 int(adj.get("relative_likelihood", 0)))
                    key = (hr.pattern, hr.window_before, hr.window_after, hr.fixed, hr.relative)
                    if key not in hot_index:
                        hot_index[key] = len(hot_rules)
                        hot_rules.append(hr)
                    for tn in tnames:
                        if tn in rules.type_id:
                            per_type_rules[rules.type_id[tn]].append(hot_index[key])
                elif "exclusion_rule" in rule:
                    ex = rule["exclusion_rule"]
                    forms = [k for k in XT_FORMS if k in ex]
                    if len(forms) != 1:
                        raise RuleError("exclusion_rule with " + (" and ".join(forms) if forms else
                                                                  "none of " + ", ".join(XT_FORMS)))
                    if forms[0] != "exclude_info_types":
                        if not text_exclusions:
                            raise RuleError(f"exclusion_rule.{forms[0]} is not supported by this call "
                                            "(compile_rules(text_exclusions=True), compile_default)")
                        tx = parse_text_exclusion(ex)
                        if tx not in xt_index:
                            xt_index[tx] = len(xt_rules)
                            xt_rules.append(tx)
                        for tn in tnames:
                            if tn in rules.type_id:
                                per_type_xt[rules.type_id[tn]].append(xt_index[tx])
                        continue
                    mt = ex.get("matching_type", "MATCHING_TYPE_FULL_MATCH")
                    if mt not in MATCHING_TYPES:
                        raise RuleError(f"exclusion_rule: unknown matching_type {mt}")
                    partial = XG_PARTIAL if mt == "MATCHING_TYPE_PARTIAL_MATCH" else 0
                    xs = [it["name"] for it in ex["exclude_info_types"].get("info_types", [])]
                    for tn in tnames:
                        if tn in rules.type_id:
                            per_type_excl[rules.type_id[tn]].extend(rules.type_id[x] | partial
                                                                    for x in xs if x in rules.type_id)
        for x in rules.external_types:
            xt = rules.type_id[x]
            if per_type_rules[xt] or per_type_excl[xt] or per_type_xt[xt] or any(xt in [i & ~XG_PARTIAL for i in l] for l in per_type_excl):
                raise RuleError(f"external type {x} cannot be named by a hotword or exclusion rule")
        for t in range(T):
            rule_ids.extend(per_type_rules[t])
            rule_off[v * T + t + 1] = len(rule_ids)
            excl_ids.extend(per_type_excl[t])
            excl_off[v * T + t + 1] = len(excl_ids)
            xt_ids.extend(per_type_xt[t])
            xt_off[v * T + t + 1] = len(xt_ids)
    # excluder patterns (their type is excluded-against in some variant) get a slot in the resolve
    # kernel's private state and come FIRST in every SCAN-D accept set, so that a same-start
    # excluder is known before the findings it may exclude (A.5).
    excluder_types = {i & ~XG_PARTIAL for i in excl_ids[:int(excl_off[-1])]}
    excluded_types = {t for v in range(V) for t in range(T) if excl_off[v * T + t + 1] > excl_off[v * T + t]}
    exidx = np.full(P, 0xFF, dtype=np.uint8)
    ne = 0
    for p in rules.patterns:
        if rules.type_id[p.type_name] in excluder_types:
            exidx[p.pid] = min(ne, 0xFE)
            ne += 1
    # GENERAL (the streaming form cannot express it): a PARTIAL_MATCH entry, more excluder patterns than
    # k_select keeps, or a type both excluded and excluding.  The lists move to var.xg_* / det.xgidx (read
    # by k_exclude, which marks the excluded candidates before k_select runs) and the streaming tables stay
    # empty.
    # ... or a rule that tests text (xt_rules): k_excl_text marks its candidates where k_exclude marks.
    general = (any(i & XG_PARTIAL for i in excl_ids) or ne > NE_MAX or bool(excluder_types & excluded_types)
               or bool(xt_rules))
    xg_sections = OrderedDict()
    window_xg_ok = 0
    if general:
        if ne > NX_MAX:
            raise RuleError(f"{ne} excluder patterns (more than {NX_MAX})")
        if T >= XG_PARTIAL:
            raise RuleError(f"{T} info types: a general exclusion list holds type ids below {XG_PARTIAL}")
        xg_sections["var.xg_off"] = excl_off
        xg_sections["var.xg_ids"] = np.array(excl_ids or [0], dtype=np.uint16)
        xg_sections["det.xgidx"] = exidx
        excl_off = np.zeros(V * T + 1, dtype=np.uint32)
        excl_ids = []
        exidx = np.full(P, 0xFF, dtype=np.uint8)
        # k_win_select's streaming exclusion cannot look ahead: windows re-scan in FULL, unless the window is
        # enabled with PII_WINDOW_XG and nothing but these rules took window_ok (window_xg_ok, meta[15])
        window_xg_ok = window_ok
        window_ok = 0
    if xt_rules:
        # text exclusion rules: per-(variant, type) rule lists, per rule (kind, window_before, window_after, 0)
        # and a HOT-form automaton in a pool of its own -- FULL / INVERSE: of \A(?:pattern)\Z, accepting
        # on the quote iff re.fullmatch does; SEARCH / HOTWORD: of the pattern (re.search)
        if len(xt_rules) > 0xFFFF:
            raise RuleError(f"{len(xt_rules)} text exclusion rules (more than {0xFFFF})")
        xt_dfas = []
        for tx in xt_rules:
            n4 = NFA()
            st = (add_whole(n4, tx.pattern, 0) if tx.kind in (XT_FULL, XT_INVERSE)
                  else add_pattern(n4, tx.pattern, 0, reverse=False))
            xt_dfas.append(build_set_dfa(n4, [st], unanchored=True))
        xt_desc, tro, flo = [], 0, 0
        for i, d in enumerate(xt_dfas):
            xt_desc.append((tro, flo, 256 * i, d.n_classes + 1, d.start[0], d.start[1], d.start[2], d.n_states))
            tro += d.trans.size
            flo += d.flags.size
        xg_sections["var.xt_off"] = xt_off
        xg_sections["var.xt_ids"] = np.array(xt_ids, dtype=np.uint16)
        xg_sections["xt.rule"] = np.array([(tx.kind, tx.window_before, tx.window_after, 0) for tx in xt_rules],
                                          dtype=np.int32).reshape(-1)
        xg_sections["xt.desc"] = np.array(xt_desc, dtype=np.int32).reshape(-1)
        xg_sections["xt.trans"] = np.concatenate([d.trans.reshape(-1) for d in xt_dfas]).astype(np.uint16)
        xg_sections["xt.flags"] = np.concatenate([d.flags for d in xt_dfas]).astype(np.uint8)
        xg_sections["xt.cmap"] = np.concatenate([d.cmap for d in xt_dfas]).astype(np.uint8)
    # one accept-set id space over all scan groups: group g's set a > 0 -> acc_base[g] + a
    acc_sets: List[Tuple[int, ...]] = [()]
    acc_base = []
    for _, m in groups:
        m.acc_sets = [tuple(sorted(s, key=lambda pid: (exidx[pid] == 0xFF, pid))) for s in m.acc_sets]
        acc_base.append(len(acc_sets) - 1)
        acc_sets.extend(m.acc_sets[1:])
    d_off = np.zeros(len(acc_sets) + 1, dtype=np.uint32)
    d_list: List[int] = []
    for i, st in enumerate(acc_sets):
        d_list.extend(st)
        d_off[i + 1] = len(d_list)
    d_ids = np.array(d_list or [0], dtype=np.uint16)

    def global_accid(g, m):
        a = m.acc_id.reshape(-1).astype(np.int64)
        return np.where(a > 0, a + acc_base[g], 0).astype(np.uint16)
    hot = []
    for hr in hot_rules:
        n3 = NFA()
        st = add_pattern(n3, hr.pattern, 0, reverse=False)
        hot.append(build_set_dfa(n3, [st], unanchored=True))
    hot_desc = np.zeros((max(1, len(hot_rules)), 4), dtype=np.int32)
    for i, hr in enumerate(hot_rules):
        hot_desc[i] = (hr.window_before, hr.window_after, hr.fixed, hr.relative)

    # ---- pools: FIRST + HOT tables in one global-memory pool ----
    pool_trans, pool_flags, pool_cmap = [], [], []
    tr_off = fl_off = cm_off = 0

    def put(d: DFA):
        nonlocal tr_off, fl_off, cm_off
        desc = (tr_off, fl_off, cm_off, d.n_classes + 1, d.start[0], d.start[1], d.start[2], d.n_states)
        pool_trans.append(d.trans.reshape(-1))
        pool_flags.append(d.flags)
        pool_cmap.append(d.cmap)
        tr_off += d.trans.size
        fl_off += d.flags.size
        cm_off += 256
        return desc

    first_desc = np.array([put(d) for d in first], dtype=np.int32).reshape(-1, 8)
    hot_dfa_desc = (np.array([put(d) for d in hot], dtype=np.int32).reshape(-1, 8) if hot
                    else np.zeros((1, 8), np.int32))
    if tr_off >= (1 << 31):
        raise RuleError("table pool too large")

    names_blob = b"".join(n.encode("ascii") + b"\0" for n in rules.type_names)
    kw_type = np.array([rules.type_id[t] for t, _, _ in rules.kw_groups] or [0], dtype=np.uint16)
    kw_always = np.array([1 if a else 0 for _, _, a in rules.kw_groups] or [0], dtype=np.uint8)
    meta = np.array([P, G, T, V,
                     scan_d.n_states, scan_d.n_classes + 1, scan_d.start,
                     scan_k.n_states, scan_k.n_classes + 1, scan_k.start,
                     len(hot_rules), min_len, scan_budget, window_ok, len(groups) - 1, window_xg_ok], dtype=np.int64)
    S = OrderedDict()
    S["meta"] = meta
    S["scan.cmap2"] = cmap2
    S["scan.d.trans"] = scan_d.trans.reshape(-1)
    S["scan.d.accid"] = global_accid(0, scan_d)
    S["scan.d.acc_off"] = d_off
    S["scan.d.acc_ids"] = d_ids
    S["scan.k.trans"] = scan_k.trans.reshape(-1)
    S["scan.k.accid"] = scan_k.acc_id.reshape(-1).astype(np.uint16)
    S["scan.k.acc_off"] = k_off
    S["scan.k.acc_ids"] = k_ids
    S["det.type"] = np.array([rules.type_id[p.type_name] for p in rules.patterns], dtype=np.uint16)
    S["det.validator"] = np.array([VALIDATOR_IDS[p.validator] for p in rules.patterns], dtype=np.uint8)
    S["det.lik"] = np.array([p.likelihood for p in rules.patterns], dtype=np.uint8)
    S["det.exidx"] = exidx
    S["det.first_desc"] = first_desc.reshape(-1)
    S["det.first_pre"] = first_pre
    S["hot.rule"] = hot_desc.reshape(-1)
    S["hot.dfa_desc"] = hot_dfa_desc.reshape(-1)
    S["pool.trans"] = np.concatenate(pool_trans).astype(np.uint16) if pool_trans else np.zeros(1, np.uint16)
    S["pool.flags"] = np.concatenate(pool_flags).astype(np.uint8) if pool_flags else np.zeros(1, np.uint8)
    S["pool.cmap"] = np.concatenate(pool_cmap).astype(np.uint8) if pool_cmap else np.zeros(256, np.uint8)
    S["var.enabled"] = var_enabled.reshape(-1)
    S["var.minlik"] = var_minlik
    S["var.rule_off"] = rule_off
    S["var.rule_ids"] = np.array(rule_ids or [0], dtype=np.uint16)
    S["var.excl_off"] = excl_off
    S["var.excl_ids"] = np.array(excl_ids or [0], dtype=np.uint16)
    S["kw.type"] = kw_type
    S["kw.always"] = kw_always
    S["types.names"] = np.frombuffer(names_blob, dtype=np.uint8).copy()
    # scan groups >= 1 (config-5 scale): (states, classes + EOT, start) + class map, table, accept ids
    if len(groups) > 1:
        S["scan.groups"] = np.array([[m.n_states, m.n_classes + 1, m.start, 0] for _, m in groups[1:]],
                                    dtype=np.int64).reshape(-1)
        for g, (_, m) in enumerate(groups[1:], start=1):
            S[f"scan.g{g}.cmap"] = m.cmap.astype(np.uint8)
            S[f"scan.g{g}.trans"] = m.trans.reshape(-1)
            S[f"scan.g{g}.accid"] = global_accid(g, m)
    # deidentify_config: per-type kind, replacement strings, mask parameters (absent: "[TYPE]" for all)
    S.update(transform_sections(rules.transforms))
    # general exclusion rules: per-(variant, type) lists with the matching bit, per-pattern excluder index;
    # text exclusion rules after them
    S.update(xg_sections)
    blob = _sections_to_blob(S)
    return Compiled(rules, scan_d, scan_k, first, hot, hot_rules, S, blob, [[p.pid for p in ps] for ps, _ in groups])


def _min_len(tree) -> int:
    def ml(items):
        return sum(one(op, av) for op, av in items)

    def one(op, av):
        if op in (C.LITERAL, C.NOT_LITERAL, C.ANY, C.IN):
            return 1
        if op == C.AT:
            return 0
        if op == C.SUBPATTERN:
            return ml(av[-1])
        if op == C.BRANCH:
            return min(ml(b) for b in av[1])
        if op in (C.MAX_REPEAT, C.MIN_REPEAT):
            return av[0] * ml(av[2])
        return 0
    return max(1, ml(list(tree)))


_CACHE: Dict[str, Compiled] = {}


def compile_default(dlp_config_path: Optional[str] = None, builtin_path: Optional[str] = None,
                    cache_dir: Optional[str] = None) -> Compiled:
    rules = Rules.load(dlp_config_path, builtin_path, fpe=True)
    # (sort_keys hides the order of the context_keywords groups, which is their priority: it is listed)
    key = hashlib.sha256(json.dumps([rules.raw, [p.__dict__ for p in rules.patterns], list(rules.context_keywords)],
                                    sort_keys=True, default=str).encode()).hexdigest()[:16]
    if key in _CACHE:
        return _CACHE[key]
    c = compile_rules(rules, text_exclusions=True)
    _CACHE[key] = c
    return c


if __name__ == "__main__":
    import time
    t0 = time.time()
    c = compile_default()
    m = c.sections["meta"]
    print(f"compiled in {time.time() - t0:.1f}s; SCAN-D {c.scan_d.n_states}x{c.scan_d.n_classes + 1} "
          f"SCAN-K {c.scan_k.n_states}x{c.scan_k.n_classes + 1} "
          f"({(c.sections['scan.d.trans'].nbytes + c.sections['scan.k.trans'].nbytes) / 1024:.1f} KiB LDS); "
          f"FIRST states {[d.n_states for d in c.first]}; HOT {[d.n_states for d in c.hot]}; "
          f"pool {c.sections['pool.trans'].nbytes / 1024:.1f} KiB; blob {len(c.blob) / 1024:.1f} KiB")
