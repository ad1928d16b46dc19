"""What the *_host calls of csrc/hdb_api.hip share is written once.

Each ranking call that answers into host memory needs a device record and its way back, a plan, the start of the call's
statistics, and -- some of them -- the exact re-run of the queries whose sampled threshold failed and the exact selection.  Each of
these has one helper; the two copies that were easy to get wrong (a re-run that reads status words the re-run itself rewrites, a
memset whose length assumes a neighbour in the workspace) cannot be copied wrongly again while these checks hold:
  * plan_topk( and hdb_launch_collect( are written once in the file;
  * the finiteness question (matrix_is_finite) is asked by the plan helper only;
  * a copy into the caller's host_record is enqueued by the close helper only;
  * one function loops over the HDB_Q_UNDERFLOW | HDB_Q_OVERFLOW words into exact topk_impl calls;
  * one function reads the clock into ht_l0 and ht_l1 round a launch.
Text checks only: no compiler, no GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = os.path.join(ROOT, "local-hyperdb_amd", "csrc", "hdb_api.hip")
PLAN, CLOSE, RERUN, BRACKET = "plan_call", "hostrec_close", "rerun_flagged", "single_launch"

_NOW = r"std::chrono::steady_clock::now\(\)"
_HOST_COPY = re.compile(r"\bhipMemcpyAsync\s*\(\s*(?:\w+\s*(?:\.|->)\s*)*host_record\b")
_FLAG_PAIR = re.compile(r"\bHDB_Q_UNDERFLOW\s*\|\s*HDB_Q_OVERFLOW\b(?!\s*\|)")
_EXACT_CALL = re.compile(r"\btopk_impl\s*\([^;]*,\s*true\s*\)\s*;")


def _strip(text):
    """Source text without comments, string / character literals and preprocessor directives (continuation lines included)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    text = re.sub(r"'(?:\\.|[^'\\\n])*'", "''", text)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)


def _bodies(code):
    """{function name: body} for every function defined at file scope of stripped source (the braces of extern "C" { },
    namespaces, structs and classes do not open a body; a lambda belongs to the function it is written in)."""
    out, cur, i = {}, [], 0
    while i < len(code):
        ch = code[i]
        if ch in ";}":
            cur = []
        elif ch == "{":
            head = "".join(cur).strip()
            cur = []
            if not (re.search(r'^(extern\s*""|namespace\b)[^()]*$', head) or re.search(r"^(template\s*<.*>\s*)?(struct|class|union)\b[^()]*$", head, re.S)):
                depth, j = 1, i + 1
                while depth:
                    depth += (code[j] == "{") - (code[j] == "}")
                    j += 1
                name = re.search(r"(\w+)\s*\(", re.sub(r"^template\s*<[^{}()]*>", "", head))
                if name:
                    assert name.group(1) not in out, f"{name.group(1)} is defined twice"
                    out[name.group(1)] = code[i + 1:j - 1]
                i = j - 1
        else:
            cur.append(ch)
        i += 1
    return out


def _where(bodies, pattern):
    pattern = re.compile(pattern) if isinstance(pattern, str) else pattern
    return {name for name, body in bodies.items() if pattern.search(body)}


def _api():
    with open(API) as fh:
        code = _strip(fh.read())
    return code, _bodies(code)


def test_the_scanner_sees_bodies_and_calls():
    code = _strip('''
    // plan_topk( in a comment; "hipMemcpyAsync(host_record" in a string below
    #define TRY(expr) do { if (expr) return fail("x"); } while \\
                      (0)
    struct Rec { void* host_record; int n = 0; };
    extern "C" {
    int hdb_a(Rec* r) { return fail("hipMemcpyAsync(host_record, 0)"); }
    }
    template <typename L>
    static inline int bracket(hdb_index* ix, L&& launch) {
        ix->ht_l0 = std::chrono::steady_clock::now();
        const int e = launch();
        ix->ht_l1 = std::chrono::steady_clock::now();
        return e;
    }
    static int close_it(const Rec& r, hipStream_t st) { if (r.n) { TRY(hipMemcpyAsync(r.host_record, r.dev, 4, st)); } return 0; }
    static int rerun(int nq) {
        for (int q = 0; q < nq; ++q) if (h[q] & (HDB_Q_UNDERFLOW | HDB_Q_OVERFLOW)) { rc = topk_impl(ix, Q + q, 1, k,
                                                                                                     stream, true); }
        return 0;
    }
    static int other(int nq) { auto f = [&] { return plan_topk(1); }; x = h & (HDB_Q_UNDERFLOW | HDB_Q_OVERFLOW | HDB_Q_NAN);
                               ix->ht_l0 = ix->ht_l1 = std::chrono::steady_clock::now(); return topk_impl(ix, Q, nq, k, stream, false); }
    ''')
    bodies = _bodies(code)
    assert sorted(bodies) == ["bracket", "close_it", "hdb_a", "other", "rerun"]
    assert len(re.findall(r"\bplan_topk\s*\(", code)) == 1 and _where(bodies, r"\bplan_topk\s*\(") == {"other"}
    assert _where(bodies, _HOST_COPY) == {"close_it"}
    assert _where(bodies, _FLAG_PAIR) == {"rerun"} and _where(bodies, _EXACT_CALL) == {"rerun"}
    assert _where(bodies, r"\bht_l0\s*=\s*" + _NOW) == {"bracket"} and _where(bodies, r"\bht_l1\s*=\s*" + _NOW) == {"bracket", "other"}


def test_plan_and_selection_are_written_once():
    code, bodies = _api()
    assert len(re.findall(r"\bplan_topk\s*\(", code)) == 1 and _where(bodies, r"\bplan_topk\s*\(") == {PLAN}
    assert len(re.findall(r"\bhdb_launch_collect\s*\(", code)) == 1
    # (the definition of matrix_is_finite is a head, not a body: only calls are found)
    assert _where(bodies, r"\bmatrix_is_finite\s*\(") == {PLAN}


def test_the_record_goes_back_through_the_close_helper():
    code, bodies = _api()
    assert _where(bodies, _HOST_COPY) == {CLOSE}
    assert len(_HOST_COPY.findall(code)) == 1


def test_one_function_reruns_flagged_queries():
    _, bodies = _api()
    loops = _where(bodies, _FLAG_PAIR) & _where(bodies, _EXACT_CALL)
    assert loops == {RERUN}
    # ... and it reads the flags off before the first re-run: the test of the words comes before the call in its text
    body = bodies[RERUN]
    assert _FLAG_PAIR.search(body).start() < _EXACT_CALL.search(body).start()
    assert len(_EXACT_CALL.findall(body)) == 1


def test_one_function_times_a_launch():
    _, bodies = _api()
    assert _where(bodies, r"\bht_l0\s*=\s*" + _NOW) == {BRACKET}
    # (hdb_topk_host resets both stamps in one chained assignment before the call: no launch between them)
    assert _where(bodies, r"\bht_l1\s*=\s*" + _NOW) == {BRACKET, "hdb_topk_host"}
    body = bodies[BRACKET]
    t0, call, t1 = (re.search(p, body) for p in (r"\bht_l0\s*=\s*" + _NOW, r"\blaunch\s*\(\s*\)", r"\bht_l1\s*=\s*" + _NOW))
    assert t0 and call and t1 and t0.start() < call.start() < t1.start()
    for user in ("run_fused", "run_bits1", "run_batch1"):
        assert re.search(r"\b%s\s*\(" % BRACKET, bodies[user]), user
