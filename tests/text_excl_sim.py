"""The text exclusion tables of a compiled blob (var.xt_* / xt.*) stepped in Python the way the engine steps
them (hot_run of csrc/pii_device.h: from the text-start state, a byte's class then the transition, an accept
flag on the state entered, the end-of-text class last).  Test infrastructure, not the reference."""
import numpy as np

XT_SEARCH, XT_FULL, XT_INVERSE, XT_HOTWORD = range(4)


class TextExclSim:
    def __init__(self, comp):
        S = comp.sections
        self.T = int(S["meta"][2])
        self.rule = S["xt.rule"].reshape(-1, 4)
        self.desc = S["xt.desc"].reshape(-1, 8)
        self.trans, self.flags, self.cmap = S["xt.trans"], S["xt.flags"], S["xt.cmap"]
        self.off, self.ids = S["var.xt_off"], S["var.xt_ids"]

    def hot_run(self, h: int, seg: bytes) -> bool:
        tr, fl, cm, nc, s0 = [int(x) for x in self.desc[h][:5]]
        st = s0
        for c in seg:
            st = int(self.trans[tr + st * nc + int(self.cmap[cm + c])])
            if self.flags[fl + st]:
                return True
        return bool(self.flags[fl + int(self.trans[tr + st * nc + nc - 1])])

    def rule_drops(self, h: int, text: bytes, s: int, e: int) -> bool:
        kind, wb, wa, _ = [int(x) for x in self.rule[h]]
        if kind == XT_HOTWORD:
            return (wb > 0 and self.hot_run(h, text[max(0, s - wb):s])) or (wa > 0 and self.hot_run(h, text[e:e + wa]))
        return self.hot_run(h, text[s:e]) != (kind == XT_INVERSE)

    def rules_of(self, v: int, t: int):
        k = v * self.T + t
        return [int(x) for x in self.ids[int(self.off[k]):int(self.off[k + 1])]]

    def drops(self, v: int, t: int, text: bytes, s: int, e: int) -> bool:
        return any(self.rule_drops(h, text, s, e) for h in self.rules_of(v, t))
