"""CPU: the environment switches the HIP library reads are exactly the ones INTEGRATION.md §4 lists."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_in_csrc():
    names, other = set(), []
    for p in sorted(glob.glob(os.path.join(ROOT, 'rec_now_amd', 'csrc', '*.[hc]pp')) + glob.glob(os.path.join(ROOT, 'rec_now_amd', 'csrc', '*.hip'))):
        text = open(p).read()
        names |= set(re.findall(r'\b(?:getenv|rn_env_int)\(\s*"(RECNOW_[A-Z0-9_]+)"', text))
        other += ['%s: %s' % (os.path.basename(p), m) for m in re.findall(r'\b(?:getenv|rn_env_int)\(\s*([^")][^,)]*)', text)
                  if not (os.path.basename(p) == 'common.hpp' and m in ('name', 'const char* name'))]      # (the helper itself)
    return names, other


def _listed():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    section = text.split('## 4. Environment switches of the library', 1)[1].split('\n## ', 1)[0]
    return re.findall(r'^\| `(RECNOW_[A-Z0-9_]+)` \|', section, flags=re.M)


def test_switches_read_by_the_library_are_listed():
    read, other = _read_in_csrc()
    listed = _listed()
    assert not other, 'environment read through a non-literal name: %s' % other
    assert len(listed) == len(set(listed)), 'INTEGRATION.md lists a switch twice'
    assert read == set(listed), 'read but not listed: %s; listed but not read: %s' % (sorted(read - set(listed)), sorted(set(listed) - read))
