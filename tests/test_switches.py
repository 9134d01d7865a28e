"""A switch a test varies inside the pytest process must not be read through a function-local static.

`static const int x = getenv("A2AMD_X") ...;` takes its value once per PROCESS: whatever the first context of the
session happened to see.  A test that then varies A2AMD_X with monkeypatch.setenv renders every parametrisation with
that first value and still passes - it no longer runs the code it is named for.  Such switches are fields of the
context, read in a2amd_open() (a2amd_host.cpp); this guard needs no library and no device.

Since then every switch of liba2amd.so is a member of one table (csrc/a2amd_switches.h) that a2amd_open() fills: the
tests below the guard hold the table to being the only reader, to the full list of names, and to the values the
scattered reads it replaced gave."""
import ast
import glob
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "audiality2_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
NAME = re.compile(r"A2AMD_[A-Z0-9_]+")


def static_switches(csrc=CSRC):
    """{switch: ["file:line", ...]} for every A2AMD_* name a `static ... = ... getenv("A2AMD_...") ...;` reads."""
    found = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        if not os.path.isfile(path):
            continue
        text = open(path, errors="replace").read()
        # (comments blanked, line numbers kept)
        text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        # a declaration that begins with `static` and runs to its `;` without opening a block
        for m in re.finditer(r"\bstatic\b[^;{}]*;", text):
            for g in re.finditer(r"getenv\s*\(\s*\"(A2AMD_[A-Z0-9_]+)\"", m.group(0)):
                line = text.count("\n", 0, m.start()) + 1       # (where the declaration begins)
                where = f"{os.path.basename(path)}:{line}"
                if where not in found.setdefault(g.group(1), []):
                    found[g.group(1)].append(where)
    return found


def _is_environ(node):
    """os.environ (or a bare `environ`)"""
    return (isinstance(node, ast.Attribute) and node.attr == "environ") or (isinstance(node, ast.Name) and node.id == "environ")


def _strings(node, skip=()):
    """every A2AMD_* name in the string constants under `node`, leaving the subtrees in `skip` out (docstrings are
    prose: only a string that IS a name, or a key of a dict, counts)"""
    out = set()
    todo = [node]
    while todo:
        n = todo.pop()
        if any(n is s for s in skip):
            continue
        if isinstance(n, ast.Constant) and isinstance(n.value, str) and NAME.fullmatch(n.value):
            out.add(n.value)
        todo.extend(ast.iter_child_nodes(n))
    return out


def _setters(fn):
    """(names set or deleted in this process by literal, True if some name is not a literal) for one function"""
    names, opaque = set(), False

    def take(arg):
        nonlocal opaque
        if isinstance(arg, ast.Constant) and isinstance(arg.value, str):
            names.update(NAME.findall(arg.value))
        else:
            opaque = True

    for n in ast.walk(fn):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute):
            f = n.func
            if f.attr in ("setenv", "delenv") and n.args:       # monkeypatch.setenv / delenv (whatever the fixture is called)
                take(n.args[0])
            elif _is_environ(f.value) and f.attr in ("setdefault", "pop", "__setitem__", "__delitem__") and n.args:
                take(n.args[0])
            elif _is_environ(f.value) and f.attr == "update":
                for a in n.args:
                    if isinstance(a, ast.Dict):
                        for k in a.keys:
                            take(k)
                    else:
                        opaque = True
                for k in n.keywords:
                    if k.arg:
                        names.update(NAME.findall(k.arg))
                    else:
                        opaque = True
        elif isinstance(n, (ast.Assign, ast.AugAssign, ast.Delete)):
            targets = n.targets if not isinstance(n, ast.AugAssign) else [n.target]
            for t in targets:
                if isinstance(t, ast.Subscript) and _is_environ(t.value):
                    take(t.slice)
    return names, opaque


def switches_set_in_process(tests=TESTS):
    """{switch: ["file::test", ...]}: the names tests/test_*.py set or delete in the pytest process itself -
    monkeypatch.setenv / delenv, writes to os.environ.  What a test hands to a child process (an env= dict, env_extra)
    is that child's first and only value and does not count.  Where a test sets a name that is not a literal (a loop over
    a table of settings), every A2AMD_* string of that function outside env= / env_extra= arguments counts."""
    found = {}
    for path in sorted(glob.glob(os.path.join(tests, "test_*.py"))):
        tree = ast.parse(open(path).read(), path)
        for fn in ast.walk(tree):
            if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                continue
            names, opaque = _setters(fn)
            if opaque:
                child = [k.value for c in ast.walk(fn) if isinstance(c, ast.Call) for k in c.keywords
                         if k.arg in ("env", "env_extra")]
                names |= _strings(fn, skip=child)
            for s in names:
                where = f"{os.path.basename(path)}::{fn.name}"
                if where not in found.setdefault(s, []):
                    found[s].append(where)
    return found


def overlap(csrc=CSRC, tests=TESTS):
    st, tv = static_switches(csrc), switches_set_in_process(tests)
    return {s: (st[s], tv[s]) for s in sorted(set(st) & set(tv))}


def test_no_test_varies_a_switch_that_is_read_once_per_process():
    bad = overlap()
    assert not bad, "switches a test varies in-process but the library reads through a function-local static:\n" + "\n".join(
        f"  {s}: read at {', '.join(src)}; set by {', '.join(tests)}" for s, (src, tests) in bad.items())


def test_the_guard_sees_what_it_is_for(tmp_path):
    """The scanners on a miniature of the defect: a static read, a literal setenv, a looped setenv over a table, a
    child-process dict that does not count, a per-call getenv that is no static."""
    csrc, tests = tmp_path / "csrc", tmp_path / "tests"
    csrc.mkdir()
    tests.mkdir()
    (csrc / "x.cpp").write_text(
        'int f(ctx *c)\n{\n'
        '\tstatic const int a = getenv("A2AMD_AA") ? atoi(getenv("A2AMD_AA")) : 0;\n'
        '\t// static const int z = getenv("A2AMD_COMMENTED") != 0;\n'
        '\tstatic const bool b = !(getenv("A2AMD_BB") &&\n\t\t\t!atoi(getenv("A2AMD_BB")));\n'
        '\tconst char *w = getenv("A2AMD_PERCALL");\n'
        '\tstatic const bool d = getenv("A2AMD_CHILD") != nullptr;\n'
        '\tstatic const bool e = getenv("A2AMD_EE") != nullptr;\n'
        '\treturn a + b + d + e + (w != 0);\n}\n')
    (tests / "test_x.py").write_text(
        'import os\n'
        'def test_literal(monkeypatch):\n'
        '    monkeypatch.setenv("A2AMD_AA", "1")\n'
        '    monkeypatch.setenv("A2AMD_PERCALL", "1")\n'
        'def test_looped(monkeypatch):\n'
        '    for tag, env in (("x", {"A2AMD_BB": "0"}),):\n'
        '        for k, v in env.items():\n'
        '            monkeypatch.setenv(k, v)\n'
        '    run(env_extra={"A2AMD_CHILD": "1"})\n'
        'def test_child_only():\n'
        '    run(env=dict(os.environ, A2AMD_CHILD="1"), env_extra={"A2AMD_CHILD": "1"})\n'
        'def test_environ():\n'
        '    os.environ["A2AMD_EE"] = "1"\n')
    assert sorted(static_switches(str(csrc))) == ["A2AMD_AA", "A2AMD_BB", "A2AMD_CHILD", "A2AMD_EE"]
    assert static_switches(str(csrc))["A2AMD_BB"] == ["x.cpp:5"]
    got = overlap(str(csrc), str(tests))
    assert sorted(got) == ["A2AMD_AA", "A2AMD_BB", "A2AMD_EE"]
    assert got["A2AMD_BB"][1] == ["test_x.py::test_looped"]


# ---------------------------------------------------------------------------
# The table: csrc/a2amd_switches.h
# ---------------------------------------------------------------------------
HEADER = os.path.join(CSRC, "a2amd_switches.h")
# every name `getenv\("A2AMD_` found in liba2amd.so's .cpp and .hip sources before the table took the reads over
SWITCHES = set("""BUS_WINDOWS CLS_CHECK COEF_CACHE_MB DBG_WALK DEBUG DEBUG_NOISE F2VPW FMVPW FVPW HOSTTIMING NOISE_QUIET NO_DIRECT
    NO_FAST NO_GRAPH NO_MOVING NO_SELFCLEAN NO_VM NZFVPG NZF_MIN NZVPW O2F_MIN RAW RECS_WPB RVPW VFILT VMSKIP VMSPEC VMSPEC_EARLY
    VMSPEC_GO VMSPEC_MIN VMWIN VM_DUMP VPW WFVPG WFWAVES WIN WIN_CHECK WIN_FORK WIN_MB WIN_MIN WIN_SLABS WIN_SYNC WIN_TIMING WVPW
    YSPLIT""".split())
# names that are not liba2amd.so's: a2amd_units.c, a2amd_walk.c, the Python side and the tests' own
ELSEWHERE = set("""WALK_OFF WALK_NOCACHE WALK_GLOBALEPOCH WALK_NOHOLD WALK_NOBLOCKS WALK_CUT WALK_STATS WALK_AHEAD WAVE_STATS DEVICE
    DEVICES BATCH NO_QUICK SPLIT NULLWALK ROOTTRACE VM_TRACE NO_RESIDENT LIB TEST_RECORD_PLAN BENCH_FORCE_DIST""".split())


def _code(path):
    """the file without its comments"""
    text = open(path, errors="replace").read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def lib_sources():
    """every file build.py's build_lib() compiles or lists as a dependency"""
    tree = ast.parse(open(os.path.join(ROOT, "audiality2_amd", "build.py")).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "build_lib")
    names = sorted({n.value for n in ast.walk(fn) if isinstance(n, ast.Constant) and isinstance(n.value, str)
                    and n.value.endswith((".cpp", ".hip", ".h"))})
    paths = [next(p for p in (os.path.join(CSRC, n), os.path.join(ROOT, "include", n)) if os.path.exists(p)) for n in names]
    return paths


def test_the_table_is_the_only_reader():
    paths = lib_sources()
    assert HEADER in paths and len(paths) > 30
    assert not [p for p in paths if os.path.basename(p) in ("a2amd_units.c", "a2amd_walk.c")]
    bad = [os.path.basename(p) for p in paths if p != HEADER and re.search(r"getenv\s*\(\s*\"A2AMD_", _code(p))]
    assert not bad, f"switches read outside a2amd_switches.h: {bad}"


def test_the_table_is_complete():
    names = set(re.findall(r"\"A2AMD_([A-Z0-9_]+)\"", _code(HEADER)))
    assert names == SWITCHES
    assert len(SWITCHES) == 45 and not SWITCHES & (ELSEWHERE - {"NO_VM", "HOSTTIMING"})
    varied = {s[len("A2AMD_"):] for s in switches_set_in_process()} - ELSEWHERE
    assert varied and varied <= names, sorted(varied - names)


#                   unset   ""    "0"   "1"   "7"  "-3"  "abc"      the read this member replaces (file:line before the table)
VALUES = (None, "", "0", "1", "7", "-3", "abc")
PARSE = {
    # presence flags: `getenv(..) != nullptr`
    "NO_MOVING": {"no_moving": (0, 1, 1, 1, 1, 1, 1)},                      # a2amd_host.cpp:67
    "NO_GRAPH": {"no_graph": (0, 1, 1, 1, 1, 1, 1)},                        # a2amd_render.cpp:153, 372 `!getenv(..)`
    # on unless 0: `!(getenv(..) && !atoi(getenv(..)))`
    "NOISE_QUIET": {"noise_quiet": (1, 0, 0, 1, 1, 1, 0)},                  # a2amd_host.cpp:68
    "WIN_FORK": {"win_fork": (1, 0, 0, 1, 1, 1, 0)},                        # a2amd_sched.cpp:1409
    "VMSPEC": {"vmspec": (1, 0, 0, 1, 1, 1, 0)},                            # a2amd_vm.cpp:865
    # int with a default: `getenv(..) ? atoi(getenv(..)) : default`
    "NO_FAST": {"no_fast": (0, 0, 0, 1, 7, -3, 0)},                         # a2amd_host.cpp:64
    "WIN_MIN": {"win_min": (2048, 0, 0, 1, 7, -3, 0)},                      # a2amd_host.cpp:72
    "O2F_MIN": {"o2f_min": (512, 0, 0, 1, 7, -3, 0)},                       # a2amd_host.cpp:70
    "VMSPEC_MIN": {"vmspec_min": (8, 0, 0, 1, 7, -3, 0)},                   # a2amd_vm.cpp:873
    "VMSKIP": {"vmskip": (1, 0, 0, 1, 7, -3, 0)},                           # a2amd_sched.cpp:1614
    "WIN_MB": {"win_mb": (1024, 0, 0, 1, 7, -3, 0)},                        # a2amd_sched.cpp:1309, a2amd_vm.cpp:881
    # ... clamped at the read: `getenv(..) ? std::max(1, atoi(getenv(..))) : default`
    "WIN_SLABS": {"win_slabs": (1, 1, 1, 1, 7, 1, 1)},                      # a2amd_host.cpp:69
    "NZF_MIN": {"nzf_min": (64, 1, 1, 1, 7, 1, 1)},                         # a2amd_host.cpp:71, a2amd_host.h:256
    # force if in range, else ignore (0: not forced)
    "RECS_WPB": {"recs_wpb": (0, 0, 0, 1, 7, 0, 0)},                        # a2amd_fast.hip:1855-1856 `force >= 1 && force <= RECS_WPB`
    "WVPW": {"wvpw": (0, 0, 0, 1, 7, 0, 0)},                                # a2amd_win.hip:1024-1025 `force > 0`
    "WFVPG": {"wfvpg": (0, 0, 0, 1, 7, 0, 0)},                              # a2amd_win.hip:1038, 1042 `force > 0`
    "WFWAVES": {"wfwaves": (0, 0, 0, 0, 7, 0, 0)},                          # a2amd_win.hip:1045-1046 `forcew > 1`
    # tri-state (-1: unset)
    "WIN": {"win": (-1, 0, 0, 1, 1, 1, 0)},                                 # a2amd_sched.cpp:1814, 1821 `wenv ? atoi(wenv) != 0 : ..`
    "VFILT": {"vfilt": (-1, 0, 0, 1, 7, -3, 0)},                            # a2amd_fast.hip:1899-1900 `fv ? atoi(fv) : -1`
    "RAW": {"raw": (-1, -1, 0, 1, 7, -3, 0)},                               # a2amd_host.cpp:179-180 `(e && *e) ? atoi(e) : -1`
    "COEF_CACHE_MB": {"coef_cache_mb": (192, 192, 0, 1, 7, -3, 0)},         # a2amd_host.cpp:179, 181 `(m && *m) ? atoi(m) : 192`
    # presence apart from the value (None: the value is not looked at while the switch is unset)
    "RVPW": {"rvpw_set": (0, 1, 1, 1, 1, 1, 1),                             # a2amd_sched.cpp:1758, a2amd_fast.hip:1902 `!getenv(..)`
             "rvpw": (None, 0, 0, 1, 7, -3, 0)},                            # a2amd_sched.cpp:1570
    "FMVPW": {"fmvpw_set": (0, 1, 1, 1, 1, 1, 1),                           # a2amd_sched.cpp:1712
              "fmvpw": (None, 0, 0, 1, 7, -3, 0)},                          # a2amd_sched.cpp:1729
    "YSPLIT": {"ysplit_set": (0, 1, 1, 1, 1, 1, 1), "ysplit": (None, 0, 0, 1, 7, -3, 0)},  # a2amd_sched.cpp:1063
    "VPW": {"vpw_set": (0, 1, 1, 1, 1, 1, 1), "vpw": (None, 0, 0, 1, 7, -3, 0)},           # a2amd_sched.cpp:1065
    # one presence bit, one level
    "HOSTTIMING": {"hosttiming": (0, 1, 1, 1, 1, 1, 1),                     # a2amd_host.cpp:65, a2amd_render.cpp:17
                   "hosttiming_level": (0, 0, 0, 1, 7, -3, 0)},             # a2amd_sched.cpp:848, a2amd_vm.cpp:913, a2amd_render.cpp:310
}


def test_the_table_parses_as_the_scattered_reads_did(tmp_path):
    probe = str(tmp_path / "switch_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", probe, os.path.join(TESTS, "switch_probe.cpp")],
                   check=True)

    def fields(env):
        out = subprocess.run([probe], env=env, check=True, capture_output=True, text=True).stdout
        return {k: int(v) for k, v in (line.split("=") for line in out.split())}

    assert set(PARSE) <= SWITCHES
    for col, val in enumerate(VALUES):
        got = fields({} if val is None else {"A2AMD_" + name: val for name in PARSE})
        assert len(got) == 45 + 8       # (eight switches have a "was set" member beside their value)
        for name, members in PARSE.items():
            for member, want in members.items():
                if want[col] is not None:
                    assert got[member] == want[col], f"A2AMD_{name}={val!r}: {member} = {got[member]}, before the table {want[col]}"
    # ... and the edges of the ranges, one by one
    got = fields({"A2AMD_WIN": "", "A2AMD_RAW": "", "A2AMD_WIN_SLABS": "0", "A2AMD_RECS_WPB": "9", "A2AMD_WFWAVES": "1",
                  "A2AMD_RVPW": "0", "A2AMD_HOSTTIMING": "0"})
    assert got["win"] == 0 and got["raw"] == -1             # "" is off for the one and unset for the other
    assert got["win_slabs"] == 1
    assert got["recs_wpb"] == 0 and got["wfwaves"] == 0     # ignored
    assert (got["rvpw_set"], got["rvpw"]) == (1, 0)
    assert (got["hosttiming"], got["hosttiming_level"]) == (1, 0)
    got = fields({"A2AMD_RECS_WPB": "8", "A2AMD_WFWAVES": "2", "A2AMD_WIN": "-3", "A2AMD_NZF_MIN": "-3"})
    assert got["recs_wpb"] == 8 and got["wfwaves"] == 2 and got["win"] == 1 and got["nzf_min"] == 1
