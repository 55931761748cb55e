"""The M2D_* environment levers: DESIGN.md section 16 ("Levers") against the sources. Text only - the test looks for
environment-variable names and nothing else, loads no library and needs no GPU.

(a) the names the package reads through its helpers (m2d_env_* of csrc/m2d_common.h, levers.* of levers.py) are the first
    column of the Levers table plus the configuration rows the package reads;
(b) no read of an M2D_* variable remains in the package outside those helpers;
(c) every M2D_* variable bench.py, tools/ or tests/ sets or reads has a row in one of the two tables;
(d) every lever of the table has an arm of tests/lever_cases.py that runs its other position, or a stated exemption."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "music2dance_amd")
NAME = r"M2D_[A-Z0-9_]+"


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _tables():
    """-> ({lever: row cells}, {configuration name: row cells}) of DESIGN.md's Levers section"""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    sec = text[text.index("\n## 16. Levers"):]
    nxt = re.search(r"\n## ", sec[4:])
    sec = sec[:nxt.start() + 4] if nxt else sec
    tables, cur = [], None
    for line in sec.splitlines():
        if line.startswith("|"):
            cells = [c.strip() for c in line.strip().strip("|").split("|")]
            if cur is None:
                cur = {}
                tables.append(cur)
            m = re.fullmatch("`(%s)`" % NAME, cells[0])
            if m:
                assert m.group(1) not in cur, "two rows for " + m.group(1)
                cur[m.group(1)] = cells[1:]
        else:
            cur = None
    assert len(tables) == 2, "the Levers section holds the lever table and the configuration table"
    return tables[0], tables[1]


def _package_sources():
    py = glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)
    c = glob.glob(os.path.join(PKG, "csrc", "*"))
    return sorted(py), sorted(p for p in c if os.path.isfile(p))


def test_table_matches_the_names_the_package_reads():
    levers, config = _tables()
    py, c = _package_sources()
    read = {}
    for p in py:
        for n in re.findall(r"levers\.(?:on|value|is_set)\(\s*\"(%s)\"" % NAME, _read(p)):
            read.setdefault(n, set()).add(os.path.relpath(p, PKG))
    for p in c:
        for n in re.findall(r"m2d_env_(?:on|int|double|raw)\(\s*\"(%s)\"" % NAME, _read(p)):
            read.setdefault(n, set()).add(os.path.relpath(p, PKG))
    assert len(read) > 40, "the scan found too few reads: has a helper been renamed?"
    config_in_package = {n for n, cells in config.items() if cells[0].startswith("`music2dance_amd/")}
    assert not (set(levers) & set(config)), "a name belongs to one table"
    assert set(read) == set(levers) | config_in_package, (
        "read but not listed: %s; listed but not read: %s"
        % (sorted(set(read) - set(levers) - config_in_package), sorted((set(levers) | config_in_package) - set(read))))
    for n, files in read.items():   # the "read in" cell names every file that reads the lever
        cell = (levers.get(n) or config[n])[0]
        for f in files:
            assert "`%s`" % f in cell or "`music2dance_amd/%s`" % f in cell, "%s is also read in %s" % (n, f)


def test_no_raw_environment_read_in_the_package():
    py, c = _package_sources()
    hits = []
    for p in py + c:
        base = os.path.basename(p)
        for i, line in enumerate(_read(p).splitlines(), 1):
            if base == "levers.py" or base == "m2d_common.h":
                # the helpers themselves: they read whatever name they are given, and name none
                if re.search(r"(getenv|environ)[^\n]*\"%s\"" % NAME, line):
                    hits.append("%s:%d" % (p, i))
            elif re.search(r"\bgetenv\b", line) or (re.search(r"\benviron\b", line) and re.search(NAME, line)):
                hits.append("%s:%d" % (p, i))
    assert not hits, "raw environment reads: " + ", ".join(hits)


def test_names_used_by_bench_tools_and_tests_are_listed():
    levers, config = _tables()
    listed = set(levers) | set(config)
    paths = [os.path.join(ROOT, "bench.py")]
    for d in ("tools", "tests"):
        paths += [p for p in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True)
                  if os.path.isfile(p) and os.path.splitext(p)[1] in (".py", ".sh", ".hip", ".h", ".cpp", ".md")]
    used = {}
    for p in paths:
        text = _read(p)
        # an environment name stands quoted (a key of os.environ, getenv's argument) or in front of `=` (a keyword of
        # dict(os.environ, ...), a shell assignment, a usage line); behind -D it is a compiler define
        for m in re.finditer(r"[\"'](%s)[\"']|(?<![A-Za-z0-9_])(?<!-D)(%s)=(?!=)" % (NAME, NAME), text):
            used.setdefault(m.group(1) or m.group(2), set()).add(os.path.relpath(p, ROOT))
    assert "M2D_LIB" in used and "M2D_MANUAL_CRITIC" in used, "the scan lost the names it is known to meet"
    missing = {n: sorted(f) for n, f in used.items() if n not in listed}
    assert not missing, "not in DESIGN.md's Levers tables: %s" % missing


def test_every_lever_has_an_arm_or_an_exemption():
    from tests import lever_cases
    levers, _ = _tables()
    in_arms = {n for a in lever_cases.ARMS.values() for n in a.env}
    exempt = set(lever_cases.EXEMPT)
    assert not (in_arms & exempt), "both an arm and an exemption: %s" % sorted(in_arms & exempt)
    assert in_arms | exempt == set(levers), ("no arm and no exemption: %s; not a lever of the table: %s"
                                            % (sorted(set(levers) - in_arms - exempt), sorted((in_arms | exempt) - set(levers))))
    assert all(isinstance(r, str) and len(r) > 10 for r in lever_cases.EXEMPT.values())
