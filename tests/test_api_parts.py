"""The parts of rucene_amd/csrc/rgpu_api.hip under csrc/api/: every part is included exactly once, and by that file alone, and
behind the first of them the file holds nothing but parts and comments. No GPU.
(While text is still being moved out of rgpu_api.hip, nothing here says that the file defines nothing itself: that assertion - no
`extern "C"` definition and no `static` function in the file - comes with the step that moves the last of it.)"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rucene_amd", "csrc")
PART_INCLUDE = re.compile(r'^\s*#\s*include\s+"(?:[^"]*/)?api/(\w+\.hpp)"', re.M)


def test_every_part_is_included_once_and_only_by_the_main_file():
    parts = sorted(f for f in os.listdir(os.path.join(CSRC, "api")))
    assert parts and all(f.endswith(".hpp") for f in parts), parts      # build() watches .hip and .hpp: another suffix would go stale
    included = PART_INCLUDE.findall(open(os.path.join(CSRC, "rgpu_api.hip")).read())
    assert sorted(included) == parts, (included, parts)                 # (a list against a list: a part included twice differs)
    # the file's own claim, "nothing else is defined from here on": from the first part on, only blank lines, // comments and parts
    lines = open(os.path.join(CSRC, "rgpu_api.hip")).read().split("\n")
    first = next(i for i, s in enumerate(lines) if s.startswith('#include "api/'))
    allowed = re.compile(r'\s*(//.*|#\s*include\s+"api/\w+\.hpp"\s*(//.*)?)?')
    assert not [s for s in lines[first:] if not allowed.fullmatch(s)]
    for d, _, files in os.walk(CSRC):
        for f in files:
            path = os.path.join(d, f)
            if path == os.path.join(CSRC, "rgpu_api.hip"):
                continue
            text = open(path, errors="replace").read()
            assert not PART_INCLUDE.search(text), path
            if d == os.path.join(CSRC, "api"):                          # a part names no sibling: `#include "x.hpp"` resolves beside it
                assert not [n for n in re.findall(r'^\s*#\s*include\s+"([^"/]+)"', text, flags=re.M) if n in parts], path

