"""Build knobs of the native library: every `ERM_*` name that an #if / #ifdef / #ifndef under csrc/ tests is a switch somebody can still flip with -D, and so a
second program nobody compiles unless a tool does.  The set is closed: the six below are used by tools/ or documented for ERM_LIB_PATH variants, and DESIGN.md
(8b) names each.  A new switch has to be added here and written down there; a settled one becomes a constant and its losing arm goes."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "extendedrtirtmodeling.jl_amd" / "csrc"

KNOBS = {"ERM_DIAG_BUILD", "ERM_DIAG_COUNTERS", "ERM_TIMELINE_BUILD", "ERM_F32_THREADS", "ERM_F64_THREADS", "ERM_F64_THREADS_LATENTQR"}
# header-local helper macros (ERM_HD, ERM_PW_FN) are defined, never tested: only names inside a conditional's expression count
CONDITIONAL = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)


def conditional_names():
    names = set()
    for f in sorted(CSRC.rglob("*")):
        if f.suffix in (".hip", ".hpp", ".h"):
            for expr in CONDITIONAL.findall(f.read_text().replace("\\\n", " ")):      # a directive continued with a backslash is one line
                names.update(re.findall(r"\bERM_[A-Z0-9_]+\b", expr))
    return names


def test_the_conditionals_test_exactly_the_documented_knobs():
    assert conditional_names() == KNOBS


def test_design_md_names_every_knob():
    text = (ROOT / "DESIGN.md").read_text()
    assert [k for k in sorted(KNOBS) if not re.search(r"\b%s\b" % k, text)] == []
