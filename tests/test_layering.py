"""The device headers' layering (diplomjourney_amd/csrc/*.h): every header
includes what it uses, the host-and-device base includes nothing above it, and
a definition precedes its use (no forward declaration of the episode update).
CPU only: host-pass syntax checks."""
import glob
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

from diplomjourney_amd import native

CSRC = os.path.join(native.PKG_DIR, "csrc")
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h")))


def _includes(path):
    """The csrc headers a header includes directly."""
    return {m for m in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M)
            if "/" not in m}


def _alone(header, tmp, *flags):
    tu = os.path.join(tmp, os.path.basename(header)[:-2] + ".hip")
    with open(tu, "w") as fh:
        fh.write(f'#include "{os.path.basename(header)}"\n')
    return subprocess.run([native.HIPCC, "--cuda-host-only", "-fsyntax-only", "-x", "hip",
                           "-std=c++17", "-I", CSRC, "-I", os.path.join(native.REPO_DIR, "include"),
                           *flags, tu], capture_output=True, text=True)


def test_device_headers_stand_alone_and_layered(tmp_path):
    assert len(HEADERS) >= 18 and os.path.join(CSRC, "mpc_device.h") in HEADERS
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        runs = list(pool.map(lambda h: _alone(h, str(tmp_path)), HEADERS))
    failed = {os.path.basename(h): r.stderr[-1500:] for h, r in zip(HEADERS, runs) if r.returncode}
    assert not failed, failed
    # what compiles for host and device sits below everything else
    assert _includes(os.path.join(CSRC, "mpc_trig.h")) == set()
    assert _includes(os.path.join(CSRC, "mpc_device.h")) == {"mpc_trig.h"}
    assert _includes(os.path.join(CSRC, "mpc_ftdevice.h")) == {"mpc_device.h"}
    # the timeline stamps sit below everything: no include at all, and the
    # header stands alone in its active form too
    timeline = os.path.join(CSRC, "mpc_timeline.h")
    assert timeline in HEADERS and "#include" not in open(timeline).read()
    active = _alone(timeline, str(tmp_path), "-DMPC_TIMELINE")
    assert active.returncode == 0, active.stderr[-1500:]
    # the episode update is defined (mpc_episode.h) before its callers: no
    # bodiless declaration of it in the headers that used to carry one
    for name in ("mpc_kernels.h", "mpc_finalize.h"):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        for fn in ("episode_hook", "episode_early_prepare"):
            assert not re.search(r"\b(void|inline)\s+" + fn + r"\s*\([^;{]*\)\s*;", text), (name, fn)
