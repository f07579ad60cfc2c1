"""A deterministic stand-in for ner.BertNer on the service path: the two capitalised words after
"my name is" are a PERSON_NAME.  Shared by the CPU and GPU service tests of the window re-scan."""
import re

NAME_RE = re.compile(rb"my name is ([A-Z][a-z]+ [A-Z][a-z]+)")


class StubNer:
    def __init__(self):
        self.calls = []

    def ext_candidates(self, texts, info_type, likelihood=4, max_len=64):
        self.calls.append(list(texts))
        return [[(m.start(1), m.end(1), info_type, likelihood) for m in NAME_RE.finditer(t)] for t in texts]
