"""Every function that crosses a translation unit of the library is declared in ONE place, csrc/hdb_launch.h.

The launchers are extern "C": a prototype that drifts from its definition still links, and the callee reads the wrong registers.
Two properties make the compiler catch that instead:
  * no prototype of an hdb_ function exists under csrc/ outside hdb_launch.h (the public ABI lives in include/hyperdb_hip.h);
  * every .hip that defines a function declared in hdb_launch.h includes that header, directly or through a header it includes,
    so a mismatch is a "conflicting types" error.
Text checks only: no compiler, no GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "local-hyperdb_amd", "csrc")
LAUNCH_H = "hdb_launch.h"


def _strip(text):
    """Source text without comments, string / character literals and preprocessor directives (continuation lines included)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    text = re.sub(r"'(?:\\.|[^'\\\n])*'", "''", text)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)


def _file_scope_statements(text):
    """(statement, terminator) for everything outside function bodies: terminator ';' for a declaration, '{' for a definition.
    The braces of extern "C" { }, namespaces, structs and classes do not open a body: what is inside them is still file scope for
    the purpose of finding prototypes."""
    out, cur, depth, transparent = [], [], 0, []
    for ch in _strip(text):
        if depth > 0:                     # inside a function body (or an initializer): skip to its end
            depth += ch == "{"
            depth -= ch == "}"
            continue
        if ch == ";":
            out.append(("".join(cur).strip(), ";"))
            cur = []
        elif ch == "{":
            head = "".join(cur).strip()
            if re.search(r'^(extern\s*""|namespace\b)[^()]*$', head) or re.search(r"^(template\s*<.*>\s*)?(struct|class|union)\b[^()]*$", head, re.S):
                transparent.append(head)
            else:
                out.append((head, "{"))
                depth = 1
            cur = []
        elif ch == "}":
            if transparent:
                transparent.pop()
            cur = []
        else:
            cur.append(ch)
    return out


_FUNC = re.compile(r"\b(hdb_\w+)\s*\(")
_DECL_MACRO = re.compile(r"\bHDB_(?:ANYD|GEOM)_DECL\s*\(\s*(hdb_\w+)\s*\)")


def _prototypes(text):
    """Names of the hdb_ functions a file declares without defining them."""
    names = []
    for stmt, end in _file_scope_statements(text):
        if end != ";" or "=" in stmt:     # (an '=' makes it an object with an initializer, not a prototype)
            continue
        m = _DECL_MACRO.search(stmt) or _FUNC.search(stmt)
        if m and not re.match(r"^(return|typedef|using)\b", stmt):
            names.append(m.group(1))
    return names


def _definitions(text):
    return [m.group(1) for stmt, end in _file_scope_statements(text) if end == "{" for m in [_FUNC.search(stmt)] if m]


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _includes(name, seen=None):
    """Headers of csrc/ that a file includes, transitively."""
    seen = set() if seen is None else seen
    for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', _read(name), flags=re.M):
        inc = os.path.basename(inc)
        if inc not in seen and os.path.exists(os.path.join(CSRC, inc)):
            seen.add(inc)
            _includes(inc, seen)
    return seen


def test_the_scanner_sees_prototypes_and_definitions():
    text = '''
    extern "C" int hdb_a(const int* p, int n);      // a prototype
    extern "C" { size_t hdb_b(void); }
    HDB_GEOM_DECL(hdb_c);
    static int x = hdb_not_this(3);
    extern "C" int hdb_d(int n) { return hdb_call(n); }
    template <typename T> static void hdb_e(T* p) { hdb_call2(p); }
    struct S { int hdb_m(int); };
    #define HDB_X(name) int name(int a, \\
                                 int b)
    '''
    assert _prototypes(text) == ["hdb_a", "hdb_b", "hdb_c", "hdb_m"]
    assert _definitions(text) == ["hdb_d", "hdb_e"]


def test_no_prototype_outside_the_launch_header():
    declared = _prototypes(_read(LAUNCH_H))
    # (66 launchers and size helpers; the capability rules the header also declared until they became inline definitions in
    # hdb_caps.h are definitions there, which the stray check below reads like any other file)
    assert len(declared) >= 60 and len(set(declared)) == len(declared), "hdb_launch.h declares each function once"
    assert "hdb_mfma_supported" in _definitions(_read("hdb_caps.h")) and not _prototypes(_read("hdb_caps.h"))
    stray = {name: _prototypes(_read(name)) for name in _sources() if name != LAUNCH_H}
    stray = {name: protos for name, protos in stray.items() if protos}
    assert not stray, f"prototypes of hdb_ functions outside {LAUNCH_H}: {stray}"


def test_every_defining_unit_sees_the_launch_header():
    declared = set(_prototypes(_read(LAUNCH_H)))
    defined = set()
    for name in _sources():
        if not name.endswith(".hip"):
            continue
        mine = declared & set(_definitions(_read(name)))
        defined |= mine
        if mine:
            assert LAUNCH_H in _includes(name), f"{name} defines {sorted(mine)} without including {LAUNCH_H}"
    assert defined == declared, f"declared in {LAUNCH_H} but defined nowhere under csrc/: {sorted(declared - defined)}"
