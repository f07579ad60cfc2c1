"""The engine's FF1 body (csrc/pii_fpe.h: ff1_apply, the text k_fpe and k_win_fpe compile) on the CPU:
tests/fpe_body_main.cpp, a stand-alone program built with the host compiler under the address and
undefined-behaviour sanitizers, transforms lines of (key record, alphabet record, finding) as the compiler
writes the records, and every output is compared with xform_fpe_ref (plain Python, big integers).

The lengths reach every path of the body: b = 12 / 13 (a second block of S) and b = 15 / 16 (a second block
of Q) lie at v = 28 / 29 for radix 10, 24 / 25 and 30 / 31 for radix 16, 16 / 17 and 20 / 21 for radix 62,
14 / 15 and 18 / 19 for radix 95; odd n gives u != v; n below nmin and above nmax fall back to '*'."""
import random
import shutil
import subprocess
import os

import pytest

import xform_fpe_ref as FR
from conftest import ROOT, pkg

SRC = os.path.join(ROOT, "tests", "fpe_body_main.cpp")
ALPHABETS = {"NUMERIC": FR.COMMON["NUMERIC"], "HEXADECIMAL": FR.COMMON["HEXADECIMAL"],
             "UPPER_CASE_ALPHA_NUMERIC": FR.COMMON["UPPER_CASE_ALPHA_NUMERIC"],
             "ALPHA_NUMERIC": FR.COMMON["ALPHA_NUMERIC"], "custom95": FR.ALPHA95, "custom2": FR.ALPHA2}
KEYS = (FR.KA, FR.KC, FR.KB)


@pytest.fixture(scope="module")
def transform(tmp_path_factory):
    """cases [(key, alphabet, finding)] -> the program's outputs, one run"""
    comp = pkg("compiler")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found (g++, c++ or clang++)"
    d = tmp_path_factory.mktemp("fpe_body")
    exe = str(d / "fpe_body_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True)
    count = [0]

    def go(cases):
        path = d / f"cases{count[0]}.txt"
        count[0] += 1
        hx = lambda b: b.hex() if b else "-"                                # noqa: E731
        recs = {}
        lines = []
        for key, alphabet, piece in cases:
            if (key, alphabet) not in recs:
                recs[key, alphabet] = (comp.fpe_key_words(key).astype("<u4").tobytes().hex(),
                                       comp.fpe_alphabet_words(alphabet).astype("<u4").tobytes().hex())
            lines.append("%s %s %s" % (*recs[key, alphabet], hx(piece)))
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [b"" if ln == "-" else bytes.fromhex(ln) for ln in r.stdout.split()]
        assert len(out) == len(cases)
        return out
    return go


def _check(transform, cases):
    got = transform(cases)
    for (key, alphabet, piece), g in zip(cases, got):
        assert g == FR.surrogate(key, alphabet, piece), (len(key), alphabet, piece)
        assert len(g) == len(piece)


def test_nist_samples_and_literals(transform):
    cases = [(k, FR.COMMON["NUMERIC"], FR.NIST_DIGITS) for k in FR.NIST_EMPTY]
    cases += [(k, FR.COMMON[a], p) for p, a, k, _ in FR.KNOWN]
    got = transform(cases)
    assert got[:3] == list(FR.NIST_EMPTY.values())
    assert got[3:] == [w for _, _, _, w in FR.KNOWN]


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_every_numeral_count(name, transform):
    """n = 0 .. nmax + 2, bare and with separators and bytes >= 0x80 between the numerals"""
    alphabet = ALPHABETS[name]
    nmin, nmax = FR.limits(len(alphabet))
    rnd = random.Random(len(alphabet))
    outside = [c for c in range(1, 256) if chr(c) not in alphabet or c >= 128]
    cases = []
    for n in range(nmax + 3):
        digits = bytes(ord(rnd.choice(alphabet)) for _ in range(n))
        key = KEYS[n % 3]
        cases.append((key, alphabet, digits))
        mixed = bytearray()
        for c in digits:
            mixed += bytes(rnd.choice(outside) for _ in range(rnd.randrange(3)))
            mixed.append(c)
        mixed += bytes(rnd.choice(outside) for _ in range(rnd.randrange(3)))
        cases.append((key, alphabet, bytes(mixed)))
    _check(transform, cases)
    fell = [FR.fallen_back(alphabet, p) for _, _, p in cases[::2]]
    assert fell == [not nmin <= n <= nmax for n in range(nmax + 3)]


def test_random_findings(transform):
    rnd = random.Random(20261)
    cases = []
    for _ in range(3000):
        alphabet = rnd.choice(list(ALPHABETS.values()))
        n = rnd.randrange(0, 90)
        piece = bytes(ord(rnd.choice(alphabet)) if rnd.random() < 0.7 else rnd.randrange(1, 256) for _ in range(n))
        cases.append((rnd.choice(KEYS), alphabet, piece))
    _check(transform, cases)


def test_all_zero_and_all_top_numerals(transform):
    """the carries: every numeral the largest, and none"""
    cases = []
    for alphabet in ALPHABETS.values():
        _, nmax = FR.limits(len(alphabet))
        for n in (nmax, nmax - 1, 7):
            cases.append((FR.KA, alphabet, alphabet[-1].encode() * n))
            cases.append((FR.KB, alphabet, alphabet[0].encode() * n))
    _check(transform, cases)
