"""The environment switches of the library are one table (amico_amd/csrc/amx_host.hpp: kSwitches), read in one place, listed in one
document.  Text checks only: no GPU, no library."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / 'amico_amd' / 'csrc'

# names handled in Python, never by the library
PYTHON_SIDE = {'AMX_DEVICES', 'AMX_PIPELINE_UNFUSED', 'AMICO_AMD_LIB'}
# AMX_* words of the C ABI that look like switches: return codes, flag bits, estimator ids, and placeholders in prose
NOT_SWITCHES = re.compile(r'AMX_(E|F|DTI|OK|ST)(_|$)|AMX_[XY]$')

ROW = re.compile(r'^\s*sw_(flag|off|given|char|int|list)\("([A-Z0-9_]+)"', re.M)


def table_rows():
    text = (CSRC / 'amx_host.hpp').read_text()
    body = text[text.index('inline constexpr amx_switch kSwitches[] = {'):]
    body = body[:body.index('\n};')]
    names = [m.group(2) for m in ROW.finditer(body)]
    assert len(names) == len(set(names)), 'a switch has two rows'
    assert len(names) >= 20
    return set(names)


def names_set_by_python():
    files = sorted((ROOT / 'tests').glob('*.py')) + [ROOT / 'bench.py', ROOT / '__graft_entry__.py'] + sorted((ROOT / 'amico_amd').glob('*.py'))
    found = {}
    for f in files:
        if f.name == 'test_switches.py':
            continue
        for name in re.findall(r'\b(?:AMX|AMICO_AMD)_[A-Z0-9_]*[A-Z0-9]\b', f.read_text()):
            if not NOT_SWITCHES.match(name):
                found.setdefault(name, f.name)
    return found


def test_every_switch_the_tree_sets_is_a_row_of_the_table():
    rows = table_rows()
    dead = {n: f for n, f in names_set_by_python().items() if n not in rows and n not in PYTHON_SIDE}
    assert not dead, f'set in Python but read by nothing in the library (retired switch?): {dead}'


def test_switches_section_lists_exactly_the_table():
    design = (ROOT / 'DESIGN.md').read_text()
    start = design.index('## 12. Switches')
    nxt = design.find('\n## ', start + 1)
    section = design[start:nxt if nxt > 0 else len(design)]
    env_part = section[:section.index('### Instrumentation build macros')]
    listed = set(re.findall(r'^\| `([A-Z0-9_]+)`', env_part, re.M))
    rows = table_rows()
    assert listed == rows, f'only in DESIGN.md: {sorted(listed - rows)}; only in amx_host.hpp: {sorted(rows - listed)}'
    macros = section[section.index('### Instrumentation build macros'):]
    for m in ('AMX_STATS', 'AMX_PHASES', 'AMX_FW_PHASES', 'AMX_LUT_PHASES', 'AMX_PEEK', 'AMX_CSRC_HASH'):
        assert f'`{m}`' in macros, m


def test_the_environment_is_read_in_one_place():
    reads = []
    for f in sorted(CSRC.glob('*.h*')):
        for k, line in enumerate(f.read_text().splitlines(), 1):
            if 'getenv(' in line:
                reads.append((f.name, k, line.strip()))
    # the table's loop in amx_ctx_create; the table justifies no other read
    assert len(reads) == 1 and reads[0][0] == 'amx_api.hip' and 'getenv(w.name)' in reads[0][2], reads
    api = (CSRC / 'amx_api.hip').read_text()
    loop = api.index('for (const amx_switch &w : kSwitches)')
    assert api.index('int amx_ctx_create(') < loop < api.index('getenv(w.name)') < api.index('void amx_ctx_destroy(')


def test_only_instrumentation_macros_gate_code():
    allowed = {'AMX_STATS', 'AMX_PHASES', 'AMX_FW_PHASES', 'AMX_LUT_PHASES', 'AMX_PEEK', 'AMX_CSRC_HASH'}
    for f in sorted(CSRC.glob('*.h*')):
        for k, line in enumerate(f.read_text().splitlines(), 1):
            m = re.match(r'#\s*if(?:n?def)?\s+(\w+)', line)
            if m:
                assert m.group(1) in allowed, f'{f.name}:{k}: {line}'
    assert '-D' not in re.sub(r'-DAMX_CSRC_HASH', '', (CSRC / 'Makefile').read_text())
