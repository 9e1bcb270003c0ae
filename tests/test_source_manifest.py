"""realism-effects_amd/csrc/sources.mk is the one list of librfx_hip.so's translation units and of the ones built with contraction on: every build
(csrc/Makefile, tests/hostsim/Makefile, tools/build_variants.sh, tools/build_combo.sh) reads it, none keeps a list of its own."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realism-effects_amd", "csrc")
# files that spell a stem because they patch that file's text (tests/hostsim/Makefile's substitutions), not because they list what to build
PATCHED = {"k3_denoise", "rfx_comm", "rfx_device"}


def manifest():
    """{variable: [words]} of sources.mk (`NAME := words`, continued with a backslash)"""
    text = open(os.path.join(CSRC, "sources.mk")).read().replace("\\\n", " ")
    text = re.sub(r"#.*", "", text)
    return {m.group(1): m.group(2).split() for m in re.finditer(r"^(\w+)\s*:=(.*)$", text, re.M)}


def test_every_hip_file_is_listed_once():
    stems = manifest()["RFX_STEMS"]
    on_disk = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted(stems) == on_disk
    assert len(set(stems)) == len(stems)


def test_contracted_files_are_sources():
    m = manifest()
    assert m["RFX_CONTRACTED"] and set(m["RFX_CONTRACTED"]) <= set(m["RFX_STEMS"])
    assert len(set(m["RFX_CONTRACTED"])) == len(m["RFX_CONTRACTED"])


def test_no_build_keeps_a_list_of_its_own():
    stems = set(manifest()["RFX_STEMS"]) - PATCHED
    for rel in ("tests/hostsim/Makefile", "tools/build_variants.sh", "tools/build_combo.sh"):
        text = open(os.path.join(ROOT, rel)).read()
        named = sorted(s for s in stems if s in text)
        assert not named, "%s names %s: the list belongs in csrc/sources.mk" % (rel, named)
