"""The host rule preparation (csrc/pii_rules_host.h) over blobs with FPE sections (xf.fpe, xf.fpe_key,
xf.fpe_alpha), on its own: the stand-alone program of test_rules_host (tests/rules_host_main.cpp, built with
the host compiler under the address and undefined-behaviour sanitizers) accepts the blobs of configs F and FC
and rejects, each defect with its own message, blobs whose sections are damaged one at a time (fpe_damage)."""
import pytest

import fpe_damage as FD
import rules_host_runner
import xform_configs as X
import xform_fpe_ref as FR
from conftest import pkg


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return rules_host_runner.runner(tmp_path_factory, "fpe_blobs")


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("fpe_cfg")
    return {n: comp.compile_default(X.write(d, n, X.with_block(b))) for n, b in (("F", FR.F), ("FC", FR.FC))}


@pytest.mark.parametrize("name", ["F", "FC"])
def test_fpe_blobs_are_accepted(name, run, blobs):
    c = blobs[name]
    out = run(name, c.blob)
    assert out.startswith("ok "), out
    assert f"types={len(c.rules.type_names)} patterns={len(c.rules.patterns)} " in out


def test_the_tables_follow_every_other_table(run, blobs, compiled):
    """rules_bytes grows by the four FPE tables alone (256-byte aligned, 16 spare bytes each), whatever the
    other tables hold: the per-type words, three key and three alphabet records, the AES table"""
    def size(out):
        return int(out.split("rules_bytes=")[1].split()[0])
    up = lambda n: (n + 255) // 256 * 256                                    # noqa: E731
    c = blobs["F"]
    S = pkg("compiler").blob_sections(c.blob)
    base = dict(S)
    for k in ("xf.fpe", "xf.fpe_key", "xf.fpe_alpha"):
        del base[k]
    kind = base["xf.kind"].copy()
    kind[kind == 6] = 4                                                      # the FPE types kept instead
    base["xf.kind"] = kind
    without = size(run("F_kept", pkg("compiler")._sections_to_blob(base)))
    T = len(c.rules.type_names)
    tables = [4 * T, 3 * 64 * 4, 3 * 68 * 4, 256 * 4]
    assert size(run("F_again", c.blob)) == up(without) + sum(up(n + 16) for n in tables[:-1]) + tables[-1] + 16


@pytest.mark.parametrize("damage, message", FD.DAMAGE, ids=FD.IDS)
def test_damaged_fpe_blob(damage, message, run, blobs):
    comp = pkg("compiler")
    S = comp.blob_sections(blobs["F"].blob)
    assert comp._sections_to_blob(S) == blobs["F"].blob                      # the round trip itself changes nothing
    damage(S)
    assert run(damage.__name__.strip("_"), comp._sections_to_blob(S)) == "rejected: " + message
