"""The offset scans that end a big scan-and-redact call: one thread of k_scan_apply does what k_finalize
did (the call's totals, the capacity test) from the two scans' totals that k_scan_blocks leaves behind
the block sums, and k_finalize is not launched.  That path (reduce / scan of sums / apply) starts above
LB_MAX_TILES x LB_TILE = 262 144 rows; below it the single-pass look-back scan and k_finalize remain.

Row counts: one row past the threshold, past it by one scan tile (2048 rows), and by a tile and five
rows.  Rows are 6-10 bytes from ten distinct texts, three of which hold an e-mail address, so the
expected offsets, totals and texts all come from the oracle's redaction of those ten texts.
"""
import functools

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

THRESH = 64 * 4096              # LB_MAX_TILES * LB_TILE (pii_engine.hip)
SCAN_TILE = 2048
COUNTS = [THRESH + 1, THRESH + SCAN_TILE, THRESH + SCAN_TILE + 5]
TEXTS = [b"a@b.io", b"me@x.com", b"jd@ab.org", b"hello!", b"ok then", b"thanks..", b"yes, sure", b"no not yet",
         b"alright", b"see you"]


@functools.lru_cache(maxsize=None)
def _table():
    """per distinct text: (redacted bytes, findings) from the oracle (CUSTOMER rows, no context)"""
    from oracle import pii_oracle as O
    cfg = O.RuleConfig.load()
    tab = [O.redact(t, cfg, None) for t in TEXTS]
    assert all(6 <= len(t) <= 10 for t in TEXTS)
    assert [len(fs) for _, fs in tab][:3] == [1, 1, 1] and not any(fs for _, fs in tab[3:])
    return tab


@pytest.fixture(scope="module")
def eng(compiled):
    e = pkg("engine").Engine(compiled.blob, device=0, n_conv_slots=16)
    yield e
    e.close()


class _Batch:
    def __init__(self, n):
        import torch
        E = pkg("engine")
        self.n = n
        rng = np.random.default_rng(n)
        self.idx = idx = rng.integers(0, len(TEXTS), n)
        tl = np.array([len(t) for t in TEXTS], dtype=np.uint64)
        offs = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(tl[idx], out=offs[1:])
        self.nb = int(offs[-1])
        data = np.zeros(self.nb + 16, dtype=np.uint8)
        for j, t in enumerate(TEXTS):
            at = offs[:-1][idx == j].astype(np.int64)
            for k, ch in enumerate(t):
                data[at + k] = ch
        tab = _table()
        ol = np.array([len(red) for red, _ in tab], dtype=np.uint64)
        self.want_offs = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(ol[idx], out=self.want_offs[1:])
        self.want_bytes = int(self.want_offs[-1])
        self.want_spans = int(np.array([len(fs) for _, fs in tab])[idx].sum())
        dev = torch.device("cuda", 0)
        self.d_text = torch.from_numpy(data).to(dev)
        self.d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        self.d_slot = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_role = torch.full((n,), E.ROLE_CUSTOMER, dtype=torch.uint8, device=dev)
        self.d_ts = torch.zeros(n, dtype=torch.int64, device=dev)
        self.d_out = torch.zeros(self.want_bytes + 64, dtype=torch.uint8, device=dev)
        self.d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.d_sp = torch.zeros((self.want_spans + 16) * 16, dtype=torch.uint8, device=dev)

    def run(self, eng, out_cap, span_cap):
        eng.scan_redact_device_ex(self.d_text.data_ptr(), self.d_offs.data_ptr(), self.n, 0, self.nb,
                                  self.d_slot.data_ptr(), self.d_role.data_ptr(), self.d_ts.data_ptr(),
                                  self.d_out.data_ptr(), out_cap, self.d_oo.data_ptr(), self.d_sp.data_ptr(), span_cap)
        return eng.sync()


@functools.lru_cache(maxsize=None)
def _batch(n):
    return _Batch(n)


@pytest.mark.parametrize("n", COUNTS)
def test_offsets_totals_and_text(eng, n):
    b = _batch(n)
    assert b.want_spans > n // 5
    ob, ns, fl = b.run(eng, b.want_bytes, b.want_spans)                 # (capacities that just suffice)
    assert (ob, ns, fl) == (b.want_bytes, b.want_spans, 0)
    got = b.d_oo.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, b.want_offs)
    out = b.d_out.cpu().numpy()
    tab = _table()
    rows = np.unique(np.concatenate([np.random.default_rng(1).integers(0, n, 996), [0, 1, n - 2, n - 1]]))
    for i in rows:
        assert out[int(got[i]):int(got[i + 1])].tobytes() == tab[int(b.idx[i])][0], i
    sp = b.d_sp.cpu().numpy()[:ns * 16].view(pkg("engine").SPAN_DTYPE)
    assert np.array_equal(sp["utt"], np.nonzero(b.idx < 3)[0])


def test_capacity_one_short(eng):
    E = pkg("engine")
    b = _batch(COUNTS[2])
    for out_cap, span_cap in ((b.want_bytes - 1, b.want_spans), (b.want_bytes, b.want_spans - 1)):
        with pytest.raises(E.PiiError) as ei:
            b.run(eng, out_cap, span_cap)
        assert ei.value.code == E.PII_E_CAPACITY
    assert b.run(eng, b.want_bytes, b.want_spans) == (b.want_bytes, b.want_spans, 0)
