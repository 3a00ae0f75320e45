"""csrc/ serves ONE instruction stream per kernel file: the only compile-time switches are the second library (WIW_F16) and
the three trace builds, and the documents advertise no -D build that the sources do not have.  Host only: text of the tree,
no compiler run."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "world-in-world_amd", "csrc")
ALLOWED = {"WIW_F16", "WIW_TRACE", "WIW_FFN_TRACE", "WIW_T_TRACE"}
CONDITIONAL = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")
NAME = re.compile(r"\b[A-Za-z_]\w*\b")


def csrc_files():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def macros_tested(path):
    """Macro names in the conditions of the #if / #ifdef / #ifndef / #elif lines of one file; an include guard
    (#ifndef X directly followed by #define X) is not a switch."""
    lines = open(path).read().split("\n")
    names = set()
    for i, line in enumerate(lines):
        m = CONDITIONAL.match(line)
        if not m:
            continue
        cond = re.sub(r"/\*.*?\*/", "", m.group(1).split("//")[0])
        found = set(NAME.findall(cond)) - {"defined"}
        nxt = lines[i + 1] if i + 1 < len(lines) else ""
        if re.match(r"^\s*#\s*ifndef\b", line) and len(found) == 1 and re.match(r"^\s*#\s*define\s+%s\s*$" % next(iter(found)), nxt):
            continue
        names |= found
    return names


def test_only_the_library_and_trace_switches_are_tested():
    files = csrc_files()
    assert len(files) >= 15, files
    extra = {os.path.basename(f): sorted(macros_tested(f) - ALLOWED) for f in files}
    extra = {f: n for f, n in extra.items() if n}
    assert not extra, f"compile-time knobs in csrc/ beyond {sorted(ALLOWED)}: {extra}"
    seen = set().union(*(macros_tested(f) for f in files))
    assert seen == ALLOWED, seen    # the parser sees the four that exist (it is not vacuously green)


def test_documents_name_only_defines_that_exist():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = re.search(r"^### 7\.1 .*?(?=^## )", design, flags=re.S | re.M)
    assert sec, "DESIGN.md has no section 7.1"
    texts = {"DESIGN.md 7.1": sec.group(0), "tools/README.md": open(os.path.join(ROOT, "tools", "README.md")).read()}
    for f in sorted(glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        texts["tools/" + os.path.basename(f)] = open(f).read()
    csrc = "\n".join(open(f).read() for f in csrc_files())
    words = set(NAME.findall(csrc))
    named = {(where, n) for where, t in texts.items() for n in re.findall(r"(?<![A-Za-z0-9])-D([A-Za-z_]\w*)", t)}
    assert ("DESIGN.md 7.1", "WIW_F16") in named and ("tools/README.md", "WIW_FFN_TRACE") in named, named
    missing = sorted((where, n) for where, n in named if n not in words)
    assert not missing, f"documents advertise -D builds that csrc/ does not have: {missing}"
