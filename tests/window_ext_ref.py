"""External candidates on the window re-scan, stated in Python: oracle.process_window_rows restated with
per-row extras (the oracle is frozen, so the statement stands beside it, as text_excl_ref.py does).

A row's external candidates -- another detector's spans (start, end, info_type, likelihood), relative to
the row, under the contract of pii_scan_redact_ext -- are produced ONCE, when the row arrives, and stay
with the row for as long as it is in its conversation's window.  The window of a row is redacted as
``O.redact(b"\\n".join(win), cfg, et, extra=joined)``, where ``joined`` holds every window entry's
candidates shifted by that entry's offset in the joined text (the sum of len + 1 over the entries before
it); a candidate therefore never crosses a "\\n".  The detector is not run over the joined text."""
from oracle import pii_oracle as O


def join_extras(win):
    """win: [(text, extras)] oldest first -> (joined text, extras in joined offsets, sorted by start)"""
    joined, off = [], 0
    for text, xs in win:
        joined += [(s + off, e + off, t, lik) for s, e, t, lik in xs]
        off += len(text) + 1
    return b"\n".join(t for t, _ in win), joined


def process_window_rows_ext(rows, extras, cfg, n=5, store=None, history=None):
    """rows as O.process_window_rows; extras[i]: row i's candidates.  history: conv -> [(text, extras)].
    Returns per row (redacted window bytes, findings in window offsets, context type used)."""
    store = store if store is not None else O.ContextStore()
    history = history if history is not None else {}
    out = []
    for (conv, role, text, ts), xs in zip(rows, extras):
        if role == O.ROLE_AGENT:
            et = O.extract_expected_pii(text, cfg)
            if et:
                store.set(conv, et, text, ts)
        win = history.setdefault(conv, [])
        win.append((text, list(xs)))
        del win[:-n]
        ctx = store.get(conv, ts)
        et = ctx[0] if ctx else None
        joined_text, joined = join_extras(win)
        red, fs = O.redact(joined_text, cfg, et, extra=joined)
        out.append((red, fs, et))
    return out
