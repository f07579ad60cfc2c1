"""pii_reidentify / pii_reidentify_device at the ABI (declared, exported, bound), and the service path that
carries findings out of process_batch and back into reidentify_batch, over an engine double whose de-identify
is the oracle's findings under xform_fpe_ref.F and whose reidentify is reid_ref."""
import os
import re

import numpy as np
import pytest

import reid_ref as RR
import xform_configs as X
import xform_fpe_ref as FR
from conftest import ROOT, pkg
from test_service import Clock, OracleEngine


def test_the_two_symbols_are_declared_exported_and_bound():
    E = pkg("engine")
    src = open(os.path.join(ROOT, "include", "pii_engine.h")).read()
    assert re.search(r"^int\s+pii_reidentify\s*\(\s*struct pii_engine\*\s*e,\s*const uint8_t\*\s*bytes,\s*"
                     r"const uint64_t\*\s*offsets,\s*uint32_t\s+n_utt,\s*const pii_span\*\s*spans,\s*uint32_t\s+n_spans,"
                     r"\s*uint8_t\*\s*out_bytes,\s*uint64_t\s+out_cap\)\s*;", src, re.M)
    assert re.search(r"^int\s+pii_reidentify_device\s*\(\s*struct pii_engine\*\s*e,\s*const uint8_t\*\s*d_bytes,\s*"
                     r"const uint64_t\*\s*d_offsets,\s*uint32_t\s+n_utt,\s*uint64_t\s+batch_base,\s*uint64_t\s+batch_bytes,"
                     r"\s*const pii_span\*\s*d_spans,\s*uint32_t\s+n_spans,\s*uint8_t\*\s*d_out_bytes,\s*"
                     r"uint64_t\s+out_cap,\s*uint32_t\*\s*d_status,\s*void\*\s*stream\)\s*;", src, re.M)
    assert re.search(r"^#define PII_REID_BAD_SPAN 1u\b", src, re.M) and re.search(r"^#define PII_REID_BAD_ARGS 2u\b", src, re.M)
    assert (E.PII_REID_BAD_SPAN, E.PII_REID_BAD_ARGS) == (1, 2)
    lib = E.load_library()
    for name, n_args in (("pii_reidentify", 8), ("pii_reidentify_device", 12)):
        assert name in E.EXPORTS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_args and fn.restype is not None
    assert hasattr(E.Engine, "reidentify") and hasattr(E.Engine, "reidentify_device")
    assert "joined window" in E.Engine.reidentify.__doc__


class FpeEngine(OracleEngine):
    """the oracle's findings, de-identified under F by xform_fpe_ref; reidentify is reid_ref"""

    def __init__(self, cfg, fail_on=None, **kw):
        super().__init__(cfg, **kw)
        self.type_names = list(cfg.type_names)
        self.config = X.with_block(FR.F)
        self.fail_on = fail_on
        self.reid_calls = []

    def scan_redact(self, texts, slots, roles, ts):
        E = pkg("engine")
        if self.fail_on is not None and any(self.fail_on in t for t in texts):
            raise E.PiiError(E.PII_E_DEVICE, "injected")
        res = super().scan_redact(texts, slots, roles, ts)
        outs, spans = [], []
        for i, t in enumerate(texts):
            et = None if res.ctx_info[i] < 0 or roles[i] != E.ROLE_CUSTOMER else self.group_types[res.ctx_info[i]]
            fs = self.O.find_pii(t, self.cfg, et)
            outs.append(FR.apply_transform(t, fs, self.type_names, self.config))
            spans += [(i, f.start, f.end, f.type_id, f.likelihood, 0) for f in fs]
        data, offs = E.pack(outs)
        return E.BatchResult(data, offs, np.array(spans, dtype=E.SPAN_DTYPE), res.ctx_info)

    def reidentify(self, texts, spans):
        E = pkg("engine")
        assert spans.dtype == E.SPAN_DTYPE
        self.reid_calls.append((list(texts), spans.copy()))
        out = []
        for u, t in enumerate(texts):
            fs = [RR.Finding(int(s["start"]), int(s["end"]), int(s["info_type"])) for s in spans[spans["utt"] == u]]
            if any(lo < 0 or hi > len(t) for lo, hi in RR.positions(fs, self.type_names, self.config)):
                raise E.PiiError(E.PII_E_ARG, "a span's output range leaves its row")
            out.append(RR.reidentify(t, fs, self.type_names, self.config))
        return out


ROWS = ["card number 4111 1111 1111 1111 ok",
        "my ssn is 536-22-1234@johnny thanks",
        "José Núñez écrit à jane.doe@corp.example.org, 4111 1111 1111 1111 — merci",
        "nothing to see here",
        "@bob_1 wrote from 10.20.30.40 call 212-555-0187 or mail jane.doe@corp.example.org"]


def _rows(texts, conv="c"):
    return [{"conversation_id": f"{conv}{i}", "participant_role": "END_USER", "text": t, "start_timestamp_usec": 10 + i}
            for i, t in enumerate(texts)]


@pytest.fixture
def svc(oracle_cfg):
    S = pkg("service")
    return S.PiiService(engine=FpeEngine(oracle_cfg, n_slots=64), clock=Clock(), time_base="payload")


def test_findings_are_names_and_byte_offsets_and_come_back(svc, oracle_cfg):
    from oracle import pii_oracle as O
    found = []
    red = svc.process_batch(_rows(ROWS), findings=found)
    assert len(found) == len(ROWS) and found[3] == []
    assert red[0] == "card number 9329 9759 1240 5582 ok" and red[1] == "my ssn is 598-59-5178 thanks"
    assert found[0] == [{"start": 12, "end": 31, "info_type": "CREDIT_CARD_NUMBER"}]
    assert found[1] == [{"start": 10, "end": 21, "info_type": "US_SOCIAL_SECURITY_NUMBER"},
                        {"start": 21, "end": 28, "info_type": "SOCIAL_HANDLE"}]
    # the non-ASCII row: offsets count bytes of the UTF-8 text, not characters
    raw = ROWS[2].encode()
    fs = O.find_pii(raw, oracle_cfg)
    assert found[2] == [{"start": f.start, "end": f.end, "info_type": oracle_cfg.type_names[f.type_id]} for f in fs]
    card = [f for f in found[2] if f["info_type"] == "CREDIT_CARD_NUMBER"][0]
    assert raw[card["start"]:card["end"]] == FR.CARD and ROWS[2][card["start"]:card["end"]] != FR.CARD.decode()
    back = svc.reidentify_batch([{"text": t, "findings": f} for t, f in zip(red, found)])
    assert back[0] == ROWS[0] and back[2] == ROWS[2] and back[3] == ROWS[3]
    assert back[1] == "my ssn is 536-22-1234 thanks"                   # the removed handle stays removed
    assert back[4] == " wrote from [IP_ADDRESS] call 212-555-0187 or mail jane.doe@corp.example.org"
    # one engine call, utt renumbered over the items that have findings
    (texts, spans), = svc.engine.reid_calls
    assert len(texts) == len(ROWS) and sorted(set(spans["utt"].tolist())) == [0, 1, 2, 4]


def test_a_failed_row_has_none_and_comes_back_unchanged(oracle_cfg):
    S = pkg("service")
    svc = S.PiiService(engine=FpeEngine(oracle_cfg, fail_on=b"nothing", n_slots=64), clock=Clock(), time_base="payload")
    found = []
    rows = _rows(ROWS)            # three engine calls, the second fails: the entries are appended call by call
    red = (svc.process_batch(rows[:3], findings=found) + svc.process_batch(rows[3:4], findings=found) +
           svc.process_batch(rows[4:], findings=found))
    assert found[3] is None and red[3] == "[DLP_API_CALL_ERROR] nothing to see here"
    assert [f is None for f in found] == [False, False, False, True, False]
    back = svc.reidentify_batch([{"text": t, "findings": f} for t, f in zip(red, found)])
    assert back[3] == red[3] and back[0] == ROWS[0]
    (texts, spans), = svc.engine.reid_calls
    assert len(texts) == 4 and sorted(set(spans["utt"].tolist())) == [0, 1, 2, 3]      # renumbered without the None
    assert svc.reidentify_batch([{"text": "x", "findings": None}]) == ["x"] and len(svc.engine.reid_calls) == 1


def test_rows_without_a_slot_have_none(oracle_cfg):
    """a run some of whose conversations get no slot (the table is at max_slots): those rows answer the error
    string and None, the others their findings, in row order"""
    S = pkg("service")
    svc = S.PiiService(engine=FpeEngine(oracle_cfg, n_slots=4), clock=Clock(), time_base="payload", max_slots=4)
    found = []
    red = svc.process_batch(_rows(ROWS), findings=found)
    assert len(found) == len(ROWS)
    lost = [i for i, f in enumerate(found) if f is None]
    assert lost and len(lost) < len(ROWS)
    for i, (r, f) in enumerate(zip(red, found)):
        assert (f is None) == r.startswith("[DLP_PROCESSING_ERROR] "), i
    assert found[0] == [{"start": 12, "end": 31, "info_type": "CREDIT_CARD_NUMBER"}]
    back = svc.reidentify_batch([{"text": t, "findings": f} for t, f in zip(red, found)])
    assert back[0] == ROWS[0] and [back[i] for i in lost] == [red[i] for i in lost]


def test_the_default_call_is_unchanged(svc, oracle_cfg):
    S = pkg("service")
    other = S.PiiService(engine=FpeEngine(oracle_cfg, n_slots=64), clock=Clock(), time_base="payload")
    found = []
    assert svc.process_batch(_rows(ROWS)) == other.process_batch(_rows(ROWS), findings=found)
    assert svc.process_batch(_rows(ROWS), None) == svc.process_batch(_rows(ROWS))
    assert svc.process_batch([], findings=found) == [] and len(found) == len(ROWS)


def test_a_bad_span_propagates(svc):
    E = pkg("engine")
    with pytest.raises(E.PiiError) as ei:
        svc.reidentify_batch([{"text": "short", "findings": [{"start": 2, "end": 40, "info_type": "CREDIT_CARD_NUMBER"}]}])
    assert ei.value.code == E.PII_E_ARG
    with pytest.raises(E.PiiError):
        svc.reidentify_batch([{"text": "short", "findings": [{"start": 0, "end": 2, "info_type": "NO_SUCH_TYPE"}]}])
