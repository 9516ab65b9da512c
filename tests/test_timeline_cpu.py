"""CPU: the timeline stamps (csrc/mpc_timeline.h) compile under -DMPC_TIMELINE,
leave no trace in the product's translation units, and every variant build
goes through native.build's compile line."""
import importlib.util
import os
import re
import subprocess

from diplomjourney_amd import native

TOOLS = os.path.join(native.REPO_DIR, "tools")
TRACES = ("g_tl", "g_tl_ep", "g_run_tl", "mpc_debug_timeline",
          "__builtin_amdgcn_s_memrealtime")


def _without_output(cmd):
    i = cmd.index("-o")
    return cmd[:i] + cmd[i + 2:]


def test_variant_translation_units_parse():
    """Both translation units, the product flags + -DMPC_TIMELINE: every stamp's
    active form (and its static_asserts: slots, table sizes) in place."""
    r = subprocess.run(native.compile_cmd(native.TIMELINE_DEFINES, os.devnull, extra=["-fsyntax-only"]),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # -Wall stays clean (the driver's own notes about link arguments aside)
    noise = [ln for ln in r.stderr.splitlines()
             if "warning" in ln and "-Wunused-command-line-argument" not in ln]
    assert not noise, noise


def test_product_translation_units_carry_no_stamp():
    """Preprocessed without the macro (host and device passes): no table, no
    clock read, no debug entry."""
    r = subprocess.run(_without_output(native.compile_cmd(extra=["-E"])), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "k_episode_chain" in r.stdout and "k_episodes_run" in r.stdout   # (both units are there)
    for name in TRACES:
        assert not re.search(r"\b" + name + r"\b", r.stdout), name
    # ... and the search does find them in the variant's
    v = subprocess.run(_without_output(native.compile_cmd(native.TIMELINE_DEFINES, extra=["-E"])),
                       capture_output=True, text=True)
    assert v.returncode == 0, v.stderr[-3000:]
    for name in TRACES:
        assert re.search(r"\b" + name + r"\b", v.stdout), name


def test_build_variant_uses_the_product_compile_line(monkeypatch, tmp_path):
    """tools/build_variant.py's compile line is native.build's, apart from the
    -D arguments, the output and the tree (argument lists compared; nothing is
    compiled)."""
    spec = importlib.util.spec_from_file_location("build_variant", os.path.join(TOOLS, "build_variant.py"))
    bv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bv)
    ran = []
    monkeypatch.setattr(native.subprocess, "run", lambda cmd, **kw: ran.append(list(cmd)))
    native.build()
    bv.main(["probe", "-DMPC_TIMELINE", "-DMPC_CHAIN_FIN_WAVES=6"])
    product, variant = ran
    assert product == native.compile_cmd() and product[-len(native.SOURCES):] == list(native.SOURCES)
    assert [a for a in variant if a.startswith("-D")] == ["-DMPC_TIMELINE", "-DMPC_CHAIN_FIN_WAVES=6"]
    assert variant[variant.index("-o") + 1] == os.path.join(TOOLS, "var_probe.so")

    def bare(cmd):
        return [a for a in _without_output(cmd) if not a.startswith("-D")]
    assert bare(variant) == bare(product)
    # another tree: the same line over that tree's files, without the units it lacks
    csrc = tmp_path / "diplomjourney_amd" / "csrc"
    csrc.mkdir(parents=True)
    (csrc / os.path.basename(native.SRC)).write_text("")
    other = native.compile_cmd(tree=str(tmp_path))
    assert [a.replace(str(tmp_path), native.REPO_DIR) for a in other] == product[:-1]
    # the timeline variant of __graft_entry__.build()
    tl = native.compile_cmd(native.TIMELINE_DEFINES, native.TIMELINE_LIB)
    assert bare(tl) == bare(product) and "-DMPC_TIMELINE" in tl
    assert tl[tl.index("-o") + 1] == os.path.join(TOOLS, "tl_variant.so")
