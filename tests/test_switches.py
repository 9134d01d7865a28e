"""A switch a test varies inside the pytest process must not be read through a function-local static.

`static const int x = getenv("A2AMD_X") ...;` takes its value once per PROCESS: whatever the first context of the
session happened to see.  A test that then varies A2AMD_X with monkeypatch.setenv renders every parametrisation with
that first value and still passes - it no longer runs the code it is named for.  Such switches are fields of the
context, read in a2amd_open() (a2amd_host.cpp); this guard needs no library and no device."""
import ast
import glob
import os
import re

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
