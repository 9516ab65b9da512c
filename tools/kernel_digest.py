"""One digest per kernel and non-inlined device function of the HIP library:
a hash of its gfx950 assembly text, so a change that claims to leave device
code alone can show it (compare two revisions' tables with diff).
    python tools/kernel_digest.py [tree | file.s]
(default: compile this tree; `tree` is any directory that holds diplomjourney_amd/csrc
and include, such as a `git archive` of another revision)
The hashed text runs from the function's `.type NAME,@function` line to its
.Lfunc_end label, comments stripped.  The function number in local labels
(.LBB<n>_, .Lfunc_end<n>) and the function's own mangled name are replaced, so
a digest depends neither on where in the file the function sits nor on what it
is called.  Text is hashed, never interpreted."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from diplomjourney_amd import native  # noqa: E402


def device_asm(tree=REPO):
    """Cross-compile the device pass of every translation unit the tree has
    (native.SOURCES by name; an older revision may have fewer) with the product
    flags; the assembly, one text, goes to a temporary directory outside the
    tree."""
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "library.s")
    with open(out, "w") as fh:
        for src in native.SOURCES:
            src = os.path.join(tree, "diplomjourney_amd", "csrc", os.path.basename(src))
            if not os.path.exists(src):
                continue
            one = os.path.join(tmp, os.path.basename(src) + ".s")
            subprocess.run([native.HIPCC, *native.HIPCC_FLAGS, "-I", os.path.join(tree, "include"),
                            "--cuda-device-only", "-S", "-o", one, src],
                           check=True, capture_output=True, cwd=tempfile.gettempdir())
            fh.write(open(one).read())
    return out


def digests(lines):
    """[(digest, mangled name)] in file order."""
    out = []
    name, body = None, []
    for raw in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", raw)
        if m:
            name, body = m.group(1), []
        if name is None:
            continue
        t = raw.split(";", 1)[0].strip()
        t = re.sub(r"\.L(BB|func_end)\d+", r".L\1", t).replace(name[2:], "@self")
        if t:
            body.append(t)
        if re.match(r"\.Lfunc_end\d*:", t):
            out.append((hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], name))
            name = None
    return out


def main():
    arg = sys.argv[1] if len(sys.argv) > 1 else REPO
    rows = digests(open(arg if arg.endswith(".s") else device_asm(arg)).read().splitlines())
    names = [n for _, n in rows]
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if filt:        # readable names where a demangler is installed
        names = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True,
                               check=True).stdout.splitlines()
    for (h, _), n in sorted(zip(rows, names), key=lambda r: r[1]):
        print(h, n)


if __name__ == "__main__":
    main()
