"""Pure-Python restatement of the incremental window re-scan under general and text exclusion rules
(PII_WINDOW_XG; k_win_lik, k_win_xmark, k_win_select with XG), over TableSim.resident_cands and the
compiled var.xg_* / var.xt_* / xt.* sections.  Test infrastructure, like tablesim.py: not the oracle.

Per window with context variant v, per entry (utterance) with resident candidates c_0 .. c_{n-1} (finditer
survivors that passed their validator, ascending start):
  lik_k        the likelihood TableSim.window_select computes: det.lik, then every hotword rule of (v, type)
               from the resident bits where known, else re-run over the joined window
  cand_k       enabled[v, type_k] and lik_k >= minlik[v]
  type_drop_k  cand_k and some g != k of the SAME entry with cand_g whose type is in the xg list of
               (v, type_k): XG_PARTIAL entry -> g.s < c.e and c.s < g.e, else g.s <= c.s and c.e <= g.e
               (g from the unfiltered list: dropped or not, it excludes)
  text_drop_k  cand_k and a rule of the xt list of (v, type_k) drops it: SEARCH / FULL / INVERSE over the
               entry's own bytes [s, e), HOTWORD over the joined window clipped to it
  c_k competes for its start iff cand_k and not type_drop_k and not text_drop_k; best per start and
  overlap resolution as TableSim.window_select.
"""
from __future__ import annotations

from tablesim import TableSim, compiler

XT_SEARCH, XT_FULL, XT_INVERSE, XT_HOTWORD = 0, 1, 2, 3


class WindowXgSim:
    def __init__(self, comp):
        self.sim = TableSim(comp)
        S = comp.sections
        assert "var.xg_off" in S, "a general rule set"
        self.xg_off, self.xg_ids = S["var.xg_off"], S["var.xg_ids"]
        self.has_xt = "var.xt_off" in S
        if self.has_xt:
            self.xt_off, self.xt_ids = S["var.xt_off"], S["var.xt_ids"]
            self.xt_rule = S["xt.rule"].reshape(-1, 4)
            self.xt_desc = S["xt.desc"].reshape(-1, 8)
            self.xt_trans, self.xt_flags, self.xt_cmap = S["xt.trans"], S["xt.flags"], S["xt.cmap"]

    # ------------------------------------------------------------------ residents of a conversation
    def residents(self, texts, n):
        """[(text, resident candidates)] of one conversation's utterances, each scanned on arrival with the
        (up to n - 1) predecessors its own window held"""
        return [(t, self.sim.resident_cands(t, texts[max(0, i - (n - 1)):i])) for i, t in enumerate(texts)]

    # ------------------------------------------------------------------ text rules
    def xt_run(self, h: int, seg: bytes) -> bool:
        tr, fl, cm, nc, st = [int(x) for x in self.xt_desc[h][:5]]
        for c in seg:
            st = int(self.xt_trans[tr + st * nc + int(self.xt_cmap[cm + c])])
            if self.xt_flags[fl + st]:
                return True
        st = int(self.xt_trans[tr + st * nc + nc - 1])
        return bool(self.xt_flags[fl + st])

    def text_drop(self, key: int, text: bytes, s: int, e: int, W: bytes, oj: int) -> bool:
        if not self.has_xt:
            return False
        for q in range(int(self.xt_off[key]), int(self.xt_off[key + 1])):
            h = int(self.xt_ids[q])
            kind, wb, wa, _ = [int(x) for x in self.xt_rule[h]]
            if kind == XT_HOTWORD:
                S, E = oj + s, oj + e
                acc = (wb > 0 and self.xt_run(h, W[max(0, S - wb):S])) or \
                      (wa > 0 and self.xt_run(h, W[E:min(len(W), E + wa)]))
            else:
                acc = self.xt_run(h, text[s:e])
            if acc != (kind == XT_INVERSE):
                return True
        return False

    # ------------------------------------------------------------------ one window
    def lik(self, cand, j, nw, text, oj, W, v):
        """lik_k, as TableSim.window_select (k_win_select's loop)"""
        sim = self.sim
        s, e, p, hot, hotx, need = cand
        t = int(sim.det_type[p])
        lik = int(sim.det_lik[p])
        known = need == 0 or j == 0 or j >= need
        bits = hot if (need == 0 or j == 0) else hotx
        for k in range(int(sim.rule_off[v * sim.T + t]), int(sim.rule_off[v * sim.T + t + 1])):
            h = int(sim.rule_ids[k])
            wb, wa, fixed, rel = [int(x) for x in sim.hot_rule[h]]
            ca = wa > 0 and e + wa > len(text) and j + 1 < nw
            ps, pe = oj + s, oj + e
            if h < sim.WHOT_BITS and known:
                hit = bool((bits >> h) & 1) or (ca and sim.hot_run(h, W[pe:pe + wa]))
            else:
                hit = (wb > 0 and sim.hot_run(h, W[max(0, ps - wb):ps])) or (wa > 0 and sim.hot_run(h, W[pe:pe + wa]))
            if hit:
                lik = fixed if fixed else min(5, max(1, lik + rel))
        return lik

    def window_select(self, entries, v: int):
        """entries = [(text, resident cands)] oldest first -> (joined window, [(start, end, type, lik)])"""
        sim = self.sim
        T = sim.T
        W = b"\n".join(t for t, _ in entries)
        nw = len(entries)
        minlik = int(sim.minlik[v])
        kept, max_end, oj = [], 0, 0
        for j, (text, cands) in enumerate(entries):
            n = len(cands)
            types = [int(sim.det_type[c[2]]) for c in cands]
            # pass 1 (k_win_lik): likelihood, candidate, text_drop
            liks = [self.lik(c, j, nw, text, oj, W, v) if sim.enabled[v, types[k]] else -1 for k, c in enumerate(cands)]
            cand = [bool(sim.enabled[v, types[k]]) and liks[k] >= minlik for k in range(n)]
            text_drop = [cand[k] and self.text_drop(v * T + types[k], text, cands[k][0], cands[k][1], W, oj)
                         for k in range(n)]
            # pass 2 (k_win_xmark): type_drop over the unfiltered candidates of this entry
            type_drop = [False] * n
            for k in range(n):
                if not cand[k]:
                    continue
                cs, ce = cands[k][0], cands[k][1]
                key = v * T + types[k]
                xs = [int(x) for x in self.xg_ids[int(self.xg_off[key]):int(self.xg_off[key + 1])]]
                for g in range(n):
                    if g == k or not cand[g]:
                        continue
                    gs, ge = cands[g][0], cands[g][1]
                    for x in xs:
                        if (x & ~compiler.XG_PARTIAL) != types[g]:
                            continue
                        if (gs < ce and cs < ge) if x & compiler.XG_PARTIAL else (gs <= cs and ce <= ge):
                            type_drop[k] = True
            # pass 3 (k_win_select): best per start, then overlap resolution
            best, s = None, -1

            def flush():
                nonlocal max_end
                if best is not None and oj + s >= max_end:
                    _, (ss, e, t, lk) = best
                    kept.append((oj + ss, oj + e, t, lk))
                    max_end = oj + e
            for k, (cs, e, p, _, _, _) in enumerate(cands):
                if cs != s:
                    flush()
                    best, s = None, cs
                if not cand[k] or type_drop[k] or text_drop[k]:
                    continue
                key = (-(e - s), -liks[k], types[k])
                if best is None or key < best[0]:
                    best = (key, (s, e, types[k], liks[k]))
            flush()
            oj += len(text) + 1
        return W, kept

    # ------------------------------------------------------------------ a stream of rows
    def process_window_rows(self, rows, ets, groups, n: int = 5):
        """rows = [(conv, role, text, ts)], ets = per row the context type its window uses (the reference's),
        groups = the context group types in order -> per row (joined window, [(start, end, type, lik)])"""
        hist, out = {}, []
        for (conv, _, text, _), et in zip(rows, ets):
            ent = hist.setdefault(conv, [])
            preds = [t for t, _ in ent[len(ent) - (n - 1):]] if n > 1 else []
            ent.append((text, self.sim.resident_cands(text, preds)))
            del ent[:-n]
            out.append(self.window_select(ent, 0 if et is None else 1 + groups.index(et)))
        return out
