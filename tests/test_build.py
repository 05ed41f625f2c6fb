"""The build recipe's header list against the sources (CPU): a header the recipe does not know is a
header whose edits rebuild nothing."""
import glob
import os
import re

from hidegs_amd import build


def test_every_quoted_include_is_a_known_header():
    known = {os.path.realpath(h) for h in build.HEADERS}
    names = {os.path.basename(h) for h in known}
    sources = [p for p in glob.glob(os.path.join(build.CSRC, "*")) if os.path.isfile(p)]
    assert sources
    missing = []
    for src in sources:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(src).read(), re.M):
            beside = os.path.join(build.CSRC, inc)
            if not os.path.isfile(beside) and os.path.basename(inc) not in names:
                missing.append((os.path.basename(src), inc))
    assert not missing, missing


def test_headers_hold_every_csrc_header():
    known = {os.path.realpath(h) for h in build.HEADERS}
    here = glob.glob(os.path.join(build.CSRC, "*.h"))
    assert here and all(os.path.realpath(h) in known for h in here)
    assert all(os.path.isfile(h) for h in build.HEADERS)
