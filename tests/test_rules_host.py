"""The host half of pii_engine_create (csrc/pii_rules_host.h) on its own, no GPU and no HIP: a small
program built with the host compiler under the address and undefined-behaviour sanitizers runs it over
the blobs the shipped compiler produces and over blobs damaged one section at a time.  The program exits
0 whether it accepts or rejects a blob; a sanitizer report is the only failure."""
import os

import pytest

import blob_damage
import rules_host_runner
from conftest import pkg


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return rules_host_runner.runner(tmp_path_factory, "blobs")


@pytest.fixture(scope="module")
def hash_compiled():
    return blob_damage.hash_config_compiled()


def test_default_config(run, compiled):
    out = run("default", compiled.blob)
    assert out.startswith("ok "), out
    assert f"types={len(compiled.rules.type_names)} " in out


def test_context_variant_config(run):
    comp = pkg("compiler")
    c = comp.compile_default(os.path.join(comp.RULES_DIR, "context_variant.json"))
    assert run("context_variant", c.blob).startswith("ok ")


def test_hash_config(run, hash_compiled):
    assert run("hash", hash_compiled.blob).startswith("ok ")


def test_not_a_blob(run):
    assert run("garbage", b"not a blob") == "rejected: not a rules blob"


@pytest.mark.parametrize("damage", blob_damage.ALL_DAMAGE, ids=blob_damage.damage_id)
def test_damaged_blob(damage, run, hash_compiled):
    out = run(blob_damage.damage_id(damage), blob_damage.damaged_blob(hash_compiled, damage))
    assert out == "rejected: " + blob_damage.MESSAGES[damage]
