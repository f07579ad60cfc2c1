"""The decrypt form of the engine's FF1 body (csrc/pii_fpe.h: ff1_apply<true>, the text k_reid compiles) on the
CPU: tests/fpe_inverse_main.cpp, a stand-alone program built with the host compiler under the address and
undefined-behaviour sanitizers and run as a program, decrypts in place (in == o) what xform_fpe_ref encrypted
and what the body itself encrypted.  Both give the finding back.  With n below nmin or above nmax the decrypt
form writes nothing: the bytes stay (reid_ref.decrypt_piece), whatever they are.

The cases are those of test_fpe_body.py, so the lengths reach every path of the body: a second block of S, a
second block of Q, u != v, and the borrows of all-zero and all-top numerals."""
import os
import random
import shutil
import subprocess

import pytest

import reid_ref as RR
import xform_fpe_ref as FR
from conftest import ROOT, pkg

SRC = os.path.join(ROOT, "tests", "fpe_inverse_main.cpp")
ALPHABETS = {"NUMERIC": FR.COMMON["NUMERIC"], "HEXADECIMAL": FR.COMMON["HEXADECIMAL"],
             "UPPER_CASE_ALPHA_NUMERIC": FR.COMMON["UPPER_CASE_ALPHA_NUMERIC"],
             "ALPHA_NUMERIC": FR.COMMON["ALPHA_NUMERIC"], "custom95": FR.ALPHA95, "custom2": FR.ALPHA2}
KEYS = (FR.KA, FR.KC, FR.KB)


@pytest.fixture(scope="module")
def inverse(tmp_path_factory):
    """cases [(key, alphabet, surrogate, finding)] -> [(surrogate decrypted, finding encrypted and decrypted)]"""
    comp = pkg("compiler")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found (g++, c++ or clang++)"
    d = tmp_path_factory.mktemp("fpe_inverse")
    exe = str(d / "fpe_inverse_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True)
    count = [0]

    def go(cases):
        path = d / f"cases{count[0]}.txt"
        count[0] += 1
        hx = lambda b: b.hex() if b else "-"                                # noqa: E731
        recs = {}
        lines = []
        for key, alphabet, sur, piece in cases:
            if (key, alphabet) not in recs:
                recs[key, alphabet] = (comp.fpe_key_words(key).astype("<u4").tobytes().hex(),
                                       comp.fpe_alphabet_words(alphabet).astype("<u4").tobytes().hex())
            lines.append("%s %s %s %s" % (*recs[key, alphabet], hx(sur), hx(piece)))
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        words = [b"" if w == "-" else bytes.fromhex(w) for w in r.stdout.split()]
        assert len(words) == 2 * len(cases)
        return list(zip(words[::2], words[1::2]))
    return go


def _check(inverse, findings):
    """findings: [(key, alphabet, finding)].  In range: the reference's surrogate and the body's own both decrypt
    to the finding.  Out of range: the finding itself is handed to the decrypt form and stays; the stars the
    encryption left stay too, unless they are n characters of the alphabet themselves (reid_ref states it)."""
    cases = []
    for key, alphabet, piece in findings:
        out = FR.fallen_back(alphabet, piece)
        cases.append((key, alphabet, piece if out else FR.surrogate(key, alphabet, piece), piece))
    got = inverse(cases)
    for (key, alphabet, sur, piece), (d1, d2) in zip(cases, got):
        if FR.fallen_back(alphabet, piece):
            assert d1 == piece, (len(key), alphabet, piece)
            stars = b"*" * len(piece)
            assert d2 == RR.decrypt_piece(key, alphabet, stars), (len(key), alphabet, piece)
            assert d2 == stars or "*" in alphabet
        else:
            assert d1 == piece, (len(key), alphabet, piece, sur)
            assert d2 == piece, (len(key), alphabet, piece)
        assert d1 == RR.decrypt_piece(key, alphabet, sur)
    return got


def test_nist_samples_and_literals(inverse):
    cases = [(k, FR.COMMON["NUMERIC"], w, FR.NIST_DIGITS) for k, w in FR.NIST_EMPTY.items()]
    cases += [(k, FR.COMMON[a], w, p) for p, a, k, w in FR.KNOWN]
    got = inverse(cases)
    for (_, _, w, p), (d1, d2) in zip(cases[:-1], got[:-1]):
        assert d1 == p and d2 == p, (p, w)
    assert FR.KNOWN[-1][0] == b"a1b" and got[-1] == (b"***", b"***")       # fail-closed stars stay stars
    _check(inverse, [(k, FR.COMMON[a], p) for p, a, k, _ in FR.KNOWN])


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_every_numeral_count(name, inverse):
    """n = 0 .. nmax + 2, bare and with separators and bytes >= 0x80 between the numerals"""
    alphabet = ALPHABETS[name]
    nmin, nmax = FR.limits(len(alphabet))
    rnd = random.Random(len(alphabet))
    outside = [c for c in range(1, 256) if chr(c) not in alphabet or c >= 128]
    findings = []
    for n in range(nmax + 3):
        digits = bytes(ord(rnd.choice(alphabet)) for _ in range(n))
        key = KEYS[n % 3]
        findings.append((key, alphabet, digits))
        mixed = bytearray()
        for c in digits:
            mixed += bytes(rnd.choice(outside) for _ in range(rnd.randrange(3)))
            mixed.append(c)
        mixed += bytes(rnd.choice(outside) for _ in range(rnd.randrange(3)))
        findings.append((key, alphabet, bytes(mixed)))
    _check(inverse, findings)
    assert [FR.fallen_back(alphabet, p) for _, _, p in findings[::2]] == [not nmin <= n <= nmax for n in range(nmax + 3)]


def test_random_findings(inverse):
    rnd = random.Random(20261)
    findings = []
    for _ in range(3000):
        alphabet = rnd.choice(list(ALPHABETS.values()))
        n = rnd.randrange(0, 90)
        piece = bytes(ord(rnd.choice(alphabet)) if rnd.random() < 0.7 else rnd.randrange(1, 256) for _ in range(n))
        findings.append((rnd.choice(KEYS), alphabet, piece))
    _check(inverse, findings)


def test_all_zero_and_all_top_numerals(inverse):
    """the borrows: every numeral the largest, and none -- as findings and as surrogates"""
    findings, raw = [], []
    for alphabet in ALPHABETS.values():
        _, nmax = FR.limits(len(alphabet))
        for n in (nmax, nmax - 1, 7):
            for key, ch in ((FR.KA, alphabet[-1]), (FR.KB, alphabet[0])):
                findings.append((key, alphabet, ch.encode() * n))
                raw.append((key, alphabet, ch.encode() * n, ch.encode() * n))
    _check(inverse, findings)
    for (key, alphabet, sur, _), (d1, _) in zip(raw, inverse(raw)):
        assert d1 == FR.surrogate(key, alphabet, sur, decrypt=True)
