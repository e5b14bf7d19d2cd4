"""The compile-time switches of csrc/ are the kept ones of docs/history/retired_switches.md, no more and no fewer.

A switch is a macro a -D on the compile line can change: every MOF_* name that a preprocessor conditional of csrc/ tests
(#ifndef, #ifdef, #if / #elif with or without defined()). Plain text scanning: no GPU, no build.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrs_optic_flow_amd", "csrc")
RECORD = os.path.join(ROOT, "docs", "history", "retired_switches.md")


def switches_of(text):
    """MOF_* names tested by the conditionals of one source text (continuation lines joined)."""
    names = set()
    for line in text.replace("\\\n", " ").splitlines():
        m = re.match(r"\s*#\s*(ifndef|ifdef|if|elif)\b(.*)", line)
        if m:
            names.update(re.findall(r"\bMOF_[A-Z0-9_]+\b", m.group(2).split("//")[0]))
    return names


def kept_switches():
    """first column of the table under '## Kept switches'"""
    section = open(RECORD).read().split("## Kept switches", 1)[1].split("\n## ", 1)[0]
    return set(re.findall(r"^\| `(MOF_[A-Z0-9_]+)` \|", section, re.M))


def test_scanner_sees_every_conditional_form():
    text = "#ifndef MOF_A  // MOF_COMMENT\n#if defined(MOF_B) && MOF_C == 2\n  #  elif !defined( MOF_D )\n#ifdef MOF_E\n#define MOF_F 1\nint x = MOF_G;\n"
    assert switches_of(text) == {"MOF_A", "MOF_B", "MOF_C", "MOF_D", "MOF_E"}


def test_csrc_carries_the_kept_switches_only():
    found = {}
    files = [f for ext in ("*.hip", "*.hpp", "*.h") for f in glob.glob(os.path.join(CSRC, ext))]
    assert len(files) > 20, "csrc not found"
    for f in files:
        for name in switches_of(open(f).read()):
            found.setdefault(name, []).append(os.path.basename(f))
    kept = kept_switches()
    assert len(kept) >= 1, "no kept switches parsed from the record"
    extra = {n: found[n] for n in sorted(set(found) - kept)}
    assert not extra, f"compile-time switches not on the keep-list of docs/history/retired_switches.md: {extra}"
    assert not kept - set(found), f"kept switches that csrc no longer tests: {sorted(kept - set(found))}"
