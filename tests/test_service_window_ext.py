"""PiiService.rescan_window_batch with a detector configured: the NEW rows' candidates reach
engine.rescan_window row for row (an engine double records them), also for the rows of a batch in which
some conversations got no slot; without a detector the call is the plain one."""
import numpy as np

from conftest import pkg
from test_service import Clock, OracleEngine
from window_ext_stub import StubNer

import window_ext_ref as WR


class _WindowExtEngine(OracleEngine):
    """Engine double with the window surface and its ext argument; results from window_ext_ref"""

    def __init__(self, cfg, n_slots=8):
        super().__init__(cfg, n_slots)
        self.type_names = list(cfg.type_names)
        self.window_n = 0
        self.hist = {}
        self.store = self.O.ContextStore()
        self.seen = []                      # per call: (texts, slots, ext or None)

    def window_enable(self, n, slot_bytes):
        self.window_n = n

    def window_reset(self, slot):
        self.hist.pop(slot, None)

    def rescan_window(self, texts, slots, roles, ts, **kw):
        E = pkg("engine")
        self.seen.append((list(texts), list(slots), kw.get("ext")))
        assert set(kw) <= {"ext"}
        ext = kw.get("ext") or [[] for _ in texts]
        ctx = self.context_update(texts, slots, roles, ts)
        out = WR.process_window_rows_ext(list(zip(slots, roles, texts, ts)), ext, self.cfg, n=self.window_n,
                                         store=self.store, history=self.hist)
        data, offs = E.pack([red for red, _, _ in out])
        return E.BatchResult(data, offs, np.zeros(0, E.SPAN_DTYPE), ctx)


def _row(cid, text, ts, role="END_USER"):
    return {"conversation_id": cid, "participant_role": role, "text": text, "start_timestamp_usec": ts}


def test_rescan_window_hands_the_detectors_lists_to_the_engine(oracle_cfg):
    S = pkg("service")
    eng, ner = _WindowExtEngine(oracle_cfg), StubNer()
    svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload", ner=ner)
    P = oracle_cfg.type_id["PERSON_NAME"]
    rows = [_row("a", "hello, my name is Jane Doe", 10), _row("a", "card 4141-1212-2323-5009", 11),
            _row("b", "my name is John Smith and my name is Al Bo", 10), _row("b", "", 11)]
    got = svc.rescan_window_batch(rows)
    texts, slots, ext = eng.seen[-1]
    assert texts == [r["text"].encode() for r in rows] and ner.calls == [texts]
    assert ext == [[(18, 26, P, 4)], [], [(11, 21, P, 4), (37, 42, P, 4)], []]
    assert got[0] == "hello, my name is [PERSON_NAME]"
    assert got[1] == "hello, my name is [PERSON_NAME]\ncard [CREDIT_CARD_NUMBER]"
    assert got[3] == "my name is [PERSON_NAME] and my name is [PERSON_NAME]\n"
    # the next call carries only its own rows' lists; the name stays in the window
    got = svc.rescan_window_batch([_row("a", "thanks", 12)])
    assert eng.seen[-1][2] == [[]]
    assert got == ["hello, my name is [PERSON_NAME]\ncard [CREDIT_CARD_NUMBER]\nthanks"]


def test_rows_without_a_slot_are_left_out_of_the_lists_too(oracle_cfg):
    S = pkg("service")
    eng, ner = _WindowExtEngine(oracle_cfg, n_slots=4), StubNer()
    svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload", ner=ner, max_slots=4)
    P = oracle_cfg.type_id["PERSON_NAME"]
    rows = [_row(f"w{c}", f"my name is Ann Lee{'x' * c}", 10) for c in range(5)]
    got = svc.rescan_window_batch(rows)
    texts, slots, ext = eng.seen[-1]
    assert len(texts) == 3 and texts == [r["text"].encode() for r in rows[:3]]       # w3, w4: no slot
    assert ext == [[(11, 18 + c, P, 4)] for c in range(3)] and ner.calls[-1] == texts
    assert got[:3] == ["my name is [PERSON_NAME]"] * 3
    assert got[3:] == [f"[DLP_PROCESSING_ERROR] {r['text']}" for r in rows[3:]]


def test_without_a_detector_the_engine_call_is_the_plain_one(oracle_cfg):
    S = pkg("service")
    eng = _WindowExtEngine(oracle_cfg)
    svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload")
    got = svc.rescan_window_batch([_row("a", "my name is Jane Doe", 10)])
    assert eng.seen[-1][2] is None and got == ["my name is Jane Doe"]
