"""The compile-time switches and the run-time knobs of csrc/ are the kept ones of docs/history/retired_switches.md, no more and no fewer.

A switch is a macro a -D on the compile line can change: every MOF_* name that a preprocessor conditional of csrc/ tests
(#ifndef, #ifdef, #if / #elif with or without defined()). A knob is an environment variable the library reads: every string literal of
csrc/ that is exactly a MOF_* name -- the argument of a getenv, or the name handed to a helper that reads it (bm_kernel.hip).
Plain text scanning: no GPU, no build.
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


def knobs_of(text):
    """String literals of one source text that are exactly a MOF_* name (a quoted name in a comment counts: write it without quotes)."""
    return set(re.findall(r'"(MOF_[A-Z0-9_]+)"', text))


def kept_knobs():
    """first column of the table under '## Kept run-time knobs', and of the table under its sub-heading '### Exempt literals'"""
    section = open(RECORD).read().split("## Kept run-time knobs", 1)[1].split("\n## ", 1)[0]
    kept, _, exempt = section.partition("### Exempt literals")
    first_column = r"^\| `(MOF_[A-Z0-9_]+)` \|"
    return set(re.findall(first_column, kept, re.M)), set(re.findall(first_column, exempt, re.M))


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


def test_scanner_sees_exact_name_literals_only():
    text = ('v = getenv("MOF_A");\nint x = env_int("MOF_B2", 1, 3);  // MOF_COMMENT\nfail("MOF_C=1 is not supported");\n'
            'puts("set MOF_D");\n#ifdef MOF_E\nconst char* n = "MOF_F_";\nconst char* l = "mof_g"; getenv("MOF_");\n')
    assert knobs_of(text) == {"MOF_A", "MOF_B2", "MOF_F_"}


def test_csrc_reads_the_kept_knobs_only():
    found = {}
    files = [f for ext in ("*.hip", "*.hpp", "*.h") for f in glob.glob(os.path.join(CSRC, ext))]
    assert len(files) > 20, "csrc not found"
    for f in files:
        for name in knobs_of(open(f).read()):
            found.setdefault(name, []).append(os.path.basename(f))
    kept, exempt = kept_knobs()
    assert len(kept) >= 1, "no kept knobs parsed from the record"
    extra = {n: found[n] for n in sorted(set(found) - kept - exempt)}
    assert not extra, f"run-time knobs not on the keep-list of docs/history/retired_switches.md: {extra}"
    assert not (kept | exempt) - set(found), f"kept knobs or exempt literals that csrc no longer holds: {sorted((kept | exempt) - set(found))}"
