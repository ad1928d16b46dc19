"""Device memory has one owner: DevBuf (csrc/hdb_devbuf.h).

tests/devbuf_check.hip, a stand-alone program with its own main, runs the type on the host under AddressSanitizer and UBSan over a
counting allocator that can fail the k-th allocation or the next copy:
    old capacity in {0, 1, 3, 64, 1000} x new capacity in {1, 3, 64, 1000, 1500} x keep in {0, 1, old} x fault in {none, 1st allocation,
    2nd allocation, copy}
for alloc (keep-nothing growth: a failure leaves the buffer empty), grow_keep (a failure leaves it as it was) and the "two locals,
then swap" pattern of buffers that change together (a failure leaves the owner as it was).  The allocator's own count of live blocks
is the leak check, at every scope exit and at program exit.
The text checks hold the rest of the library to it: with comments and strings stripped, hdb_api.hip names no hipMalloc / hipFree,
hdb_devbuf.h is the only file under csrc/ that does, and the pinned host buffers of the group (another allocator) are allocated in
group_pinned and freed there and in hdb_group_destroy only.  No GPU is used."""
import os
import re

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "local-hyperdb_amd", "csrc")
DEVBUF_H = "hdb_devbuf.h"
_DEVICE = re.compile(r"\bhip(?:Malloc|Free)\w*")          # (hipHostMalloc / hipHostFree do not start like this)
_PINNED = re.compile(r"\bhipHost(?:Malloc|Free)\b")


def _strip(text):
    """Source text without comments and string / character literals."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"'(?:\\.|[^'\\\n])*'", "''", text)


def _code(name):
    with open(os.path.join(CSRC, name)) as fh:
        return _strip(fh.read())


def _without_body(text, func):
    """-> (text without the body of the definition of `func`, that body)."""
    m = re.search(r"\b%s\s*\([^;{}]*\)\s*\{" % re.escape(func), text)
    assert m, f"no definition of {func}"
    depth, i = 1, m.end()
    while depth:
        depth += (text[i] == "{") - (text[i] == "}")
        i += 1
    return text[:m.end()] + text[i - 1:], text[m.end():i - 1]


def test_devbuf_over_a_counting_allocator(tmp_path):
    out = host_check.run(host_check.build("devbuf_check", tmp_path))


def test_the_scanner_sees_calls_and_bodies():
    text = _strip('''
    // hipFree(a) in a comment
    static int f(char** p) { if (x) { hipHostFree(*p); } return fail("hipMalloc failed"); }
    static int g(void* q) { return hipMallocAsync(&q, 4, 0) + hipFree(q); }
    ''')
    assert _DEVICE.findall(text) == ["hipMallocAsync", "hipFree"]
    rest, body = _without_body(text, "f")
    assert _PINNED.findall(body) == ["hipHostFree"] and not _PINNED.search(rest) and "hipFree" in rest


def test_device_memory_is_allocated_and_freed_in_one_header():
    sources = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert DEVBUF_H in sources and "hdb_api.hip" in sources
    assert not _DEVICE.search(_code("hdb_api.hip")), "hdb_api.hip allocates or frees device memory itself"
    users = [name for name in sources if _DEVICE.search(_code(name))]
    assert users == [DEVBUF_H], f"device allocation calls under csrc/: {users}"
    assert {"hipMalloc", "hipFree"} <= set(_DEVICE.findall(_code(DEVBUF_H)))


def test_pinned_host_memory_stays_with_the_group():
    api = _code("hdb_api.hip")
    api, pinned = _without_body(api, "group_pinned")
    api, destroy = _without_body(api, "hdb_group_destroy")
    assert set(_PINNED.findall(pinned)) == {"hipHostMalloc", "hipHostFree"}
    assert set(_PINNED.findall(destroy)) == {"hipHostFree"}
    assert not _PINNED.search(api), "pinned host memory outside group_pinned / hdb_group_destroy"
    others = [name for name in os.listdir(CSRC) if name.endswith((".hip", ".h")) and name != "hdb_api.hip" and _PINNED.search(_code(name))]
    assert not others, f"pinned host allocation calls outside hdb_api.hip: {others}"
