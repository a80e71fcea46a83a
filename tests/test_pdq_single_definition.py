"""The PDQ path's bit-exact device arithmetic has one definition, in csrc/hvd_pdq_dev.h.

The contract is "this exact sequence of roundings" (oracle/hvd_oracle.c), and copies of a sequence drift apart one edit at
a time. Four kernel files once carried their own copies of the luma, the quality term, the median select and the box-filter
line pass; this module keeps them from coming back. It reads source text only: no compiler, no GPU.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
HEADER = "hvd_pdq_dev.h"
KERNEL_FILES = ("k_pdq.hip", "k_pdq_dihedral.hip", "k_autocrop.hip", "k_autocrop_fused.hip")


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert os.path.join(CSRC, HEADER) in paths
    return {os.path.basename(p): open(p).read() for p in paths}


def _code(text):
    """The text without // comments (the derivations speak of the names they explain)."""
    return "\n".join(re.sub(r"//.*", "", ln) for ln in text.splitlines())


def _occurrences(literal):
    """file -> count over the raw text, comments included"""
    return {name: text.count(literal) for name, text in _sources().items() if literal in text}


def test_luma_weights_live_in_the_header_only():
    assert _occurrences("0.299f") == {HEADER: 1}


def test_helpers_are_defined_exactly_once():
    for name in ("grad_term", "grad_term_gray", "wave_median256", "wave_lds_handover", "wave_next_lane", "byte_of"):
        # a definition or declaration: a return type, the name, an opening parenthesis and a typed first parameter (or none)
        pat = re.compile(r"\b(?:void|float|int|uint32_t)\s+%s\s*\(\s*(?:\)|const\b|float\b|int\b|uint32_t\b)" % name)
        found = {f: len(pat.findall(_code(t))) for f, t in _sources().items() if pat.search(_code(t))}
        assert found == {HEADER: 1}, (name, found)
    found = {f: len(re.findall(r"\bconstexpr\s+int\s+kRing\b", _code(t))) for f, t in _sources().items()}
    assert {f: n for f, n in found.items() if n} == {HEADER: 1}, found


def test_select_and_divisor_choice_are_written_once():
    assert _occurrences("remaining == 1") == {HEADER: 1}
    assert _occurrences("(cur & (cur - 1)) == 0") == {HEADER: 1}


def test_kernel_files_include_the_header():
    src = _sources()
    for f in KERNEL_FILES:
        assert '#include "%s"' % HEADER in src[f], f
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^%\.o: %\.hip .*\bhvd_pdq_dev\.h\b", mk, re.M)
