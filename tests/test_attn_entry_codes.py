"""The argument errors of every launching attention entry point (attn_batch.hip, attn_prefill.hip, attn_ragged.hip,
attn_prefill_wide.hip) and their precedence, without a GPU: a fixed table of bad-argument calls with made-up addresses, never a
buffer, held to the codes recorded in tests/golden/attn_entry_codes.json.

    python tests/test_attn_entry_codes.py --record      # re-records the golden file from the library as built

The golden file is a record of what the entry points answered BEFORE a change of their host side: a refactor of the launch path
leaves it alone.  Every case is refused on the host (a code < 0), so none of them can launch."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_entry_codes.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import qpalette_amd as qp  # noqa: E402

NQ, NKV, HD, LEN = 32, 8, 128, 1024  # rep 4; a cache of 1024 positions: every launch of it needs a workspace
PTR = 1 << 16                        # the made-up address of every pointer argument: aligned to anything

_QKV = ["q", "k", "v", "ld_qkv", "kcache", "vcache", "out", "ld_out"]
_PAGES = ["table", "ld_table", "num_pages", "page_size", "max_pages", "kv_fmt"]
_ROW_PAGES = [a for a in _PAGES if a != "ld_table"]  # one sequence: a block-table row
_TAIL = ["ws", "ws_bytes", "stream"]
_HEADS = ["nq", "nkv", "hd"]
_SEG = ["seq", "row0", "pos"]
_RSB = ["rows", "S", "B"]

# entry point -> (its arguments in order, the function that sizes its workspace)
ENTRIES = {
    "decode_batch": (_QKV + ["pos", "inv_freq", "rows"] + _HEADS + ["max_len", "scale"] + _TAIL, "batch"),
    "decode_batch_kv8": (_QKV + ["pos", "inv_freq", "rows"] + _HEADS + ["max_len", "scale"] + _TAIL, "batch"),
    "decode_batch_paged": (_QKV + ["pos", "inv_freq"] + _PAGES + ["rows"] + _HEADS + ["scale"] + _TAIL, "batch"),
    "decode_batch_window": (_QKV + ["pos", "inv_freq"] + _PAGES + ["rows"] + _HEADS + ["max_len", "scale", "window"] + _TAIL, "batch"),
    "decode_batch_score": (_QKV + ["pos", "inv_freq"] + _PAGES + ["rows"] + _HEADS + ["max_len", "scale", "window", "softcap", "sinks"]
                           + _TAIL, "batch"),
    "decode_batch_shared": (_QKV + ["pos", "inv_freq"] + _PAGES + ["row_group", "grp_slot", "grp_len", "G", "rows"] + _HEADS + ["scale"]
                            + _TAIL, "prefix"),
    "prefill": (_QKV + ["pos", "inv_freq", "rows"] + _HEADS + ["max_len", "scale"] + _TAIL, "prefill"),
    "prefill_kv8": (_QKV + ["pos", "inv_freq", "rows"] + _HEADS + ["max_len", "scale"] + _TAIL, "prefill"),
    "prefill_paged": (_QKV + ["pos", "inv_freq"] + _ROW_PAGES + ["rows"] + _HEADS + ["scale"] + _TAIL, "prefill"),
    "prefill_window": (_QKV + ["pos", "inv_freq"] + _ROW_PAGES + ["rows"] + _HEADS + ["max_len", "scale", "window"] + _TAIL, "prefill"),
    "prefill_score": (_QKV + ["pos", "inv_freq"] + _ROW_PAGES + ["rows"] + _HEADS + ["max_len", "scale", "window", "softcap", "sinks"]
                      + _TAIL, "prefill"),
    "prefill_wide": (_QKV + ["pos", "inv_freq"] + _ROW_PAGES + ["rows"] + _HEADS + ["max_len", "scale"] + _TAIL, "prefill_wide"),
    "prefill_ragged": (_QKV + _SEG + ["inv_freq", "kv_fmt"] + _RSB + _HEADS + ["max_len", "scale"] + _TAIL, "ragged"),
    "prefill_ragged_paged": (_QKV + _SEG + ["inv_freq"] + _PAGES + _RSB + _HEADS + ["scale"] + _TAIL, "ragged"),
    "prefill_ragged_tree": (_QKV + _SEG + ["depth", "anc", "inv_freq", "kv_fmt"] + _RSB + _HEADS + ["max_len", "scale"] + _TAIL, "ragged"),
    "prefill_ragged_tree_paged": (_QKV + _SEG + ["depth", "anc", "inv_freq"] + _PAGES + _RSB + _HEADS + ["scale"] + _TAIL, "ragged"),
    "prefill_ragged_window": (_QKV + _SEG + ["inv_freq"] + _PAGES + _RSB + _HEADS + ["max_len", "scale", "window"] + _TAIL, "ragged"),
    "prefill_ragged_score": (_QKV + _SEG + ["inv_freq"] + _PAGES + _RSB + _HEADS + ["max_len", "scale", "window", "softcap", "sinks"]
                             + _TAIL, "ragged"),
}

POINTERS = ("q", "k", "v", "kcache", "vcache", "out", "pos", "inv_freq", "seq", "row0", "depth", "anc", "table", "row_group", "grp_slot",
            "grp_len", "sinks", "ws")
# how far off each pointer is pushed: one step below the alignment its check asks for
OFF = {"kcache": 8, "vcache": 8, "out": 1, **{p: 2 for p in POINTERS if p not in ("kcache", "vcache", "out")}}


def _ws_bytes(lib, sizer, a):
    """the bytes the launch of arguments `a` needs, from the library's own sizers (the windows of this table are 0 or >= max_len:
    the launch is sized as the one without a window)"""
    shape = (a["nq"], a["nkv"], a["hd"], LEN)
    if sizer == "batch":
        return lib.qpal_attn_batch_ws_bytes(a["rows"], *shape)
    if sizer == "prefix":
        return lib.qpal_attn_prefix_ws_bytes(a["rows"], a["G"], *shape)
    if sizer == "ragged":
        return lib.qpal_attn_ragged_ws_bytes(a["rows"], a["S"], *shape)
    return getattr(lib, f"qpal_attn_{sizer}_ws_bytes")(a["rows"], *shape)


def _flavours(entry, order):
    """(name, overrides of the base arguments): the ways into an entry point that take different paths through its preamble"""
    caches = [("", {})]
    if entry.endswith(("_window", "_score", "_wide")):  # a null table: contiguous caches
        caches = [("contig", {"table": None, "ld_table": 0, "num_pages": 0, "page_size": 0, "max_pages": 0}), ("paged", {})]
    mods = [("", {})]
    if "softcap" in order:
        mods = [("w0", {}), ("cap_w0", {"softcap": 30.0, "sinks": PTR}), ("cap_wmax", {"softcap": 30.0, "sinks": PTR, "window": LEN}),
                ("sinks_only", {"sinks": PTR})]
    elif "window" in order:
        mods = [("w0", {}), ("wmax", {"window": LEN})]
    return [("_".join(x for x in (c, m) if x), {**co, **mo}) for c, co in caches for m, mo in mods]


def _cases(entry, order, base):
    """(name, overrides) of the bad-argument cases of one flavour of one entry point"""
    has = lambda *names: all(n in order for n in names)  # noqa: E731
    paged = has("table") and base["table"] is not None
    wide = entry == "prefill_wide"
    table_optional = entry.endswith(("_window", "_score", "_wide"))
    ptrs = [p for p in POINTERS if has(p) and base[p] is not None]
    out = []
    add = lambda name, **kw: out.append((name, kw))  # noqa: E731
    for p in ptrs:
        if not (p == "table" and table_optional) and p != "sinks":  # (those two: null is "none", no fault)
            add(f"null_{p}", **{p: None})
        add(f"misaligned_{p}", **{p: PTR + OFF[p]})
    if wide:
        add("misaligned_ws_by_4", ws=PTR + 4)
    if has("kv_fmt"):
        add("kv_fmt_2", kv_fmt=2)
    if paged:
        add("page_size_17", page_size=17)
        add("num_pages_0", num_pages=0)
        add("max_pages_0", max_pages=0)
        if has("ld_table"):
            add("ld_table_short", ld_table=base["max_pages"] - 1)
        add("kv_fmt_2_page_size_17", kv_fmt=2, page_size=17)
    if has("window"):
        add("window_neg", window=-1)
        add("window_neg_kv_fmt_2", window=-1, kv_fmt=2)
        add("null_q_window_neg", q=None, window=-1)
    if has("softcap"):
        for name, val in (("neg", -1.0), ("nan", math.nan), ("inf", math.inf)):
            add(f"softcap_{name}", softcap=val)
        add("softcap_neg_kv_fmt_2", softcap=-1.0, kv_fmt=2)
        if base["sinks"] is not None:
            add("misaligned_sinks_ws_bytes_short", sinks=PTR + 2, ws_bytes=base["ws_bytes"] - 1)
    for r in ((128, 257) if wide else (0, 129)):
        add(f"rows_{r}", rows=r)
    if has("S"):
        add("S_0", S=0)
        add("S_129", S=129)
        add("B_0", B=0)
    if has("G"):
        add("G_0", G=0)
        add("G_17", G=17)
    add("hd_96", hd=96, ld_qkv=NQ * 96, ld_out=NQ * 96)
    add("nkv_0", nkv=0)  # (a code, not a division by zero: the shape rule comes before nq / nkv is formed)
    add("nq_0", nq=0)
    add("rep_3", nq=24, ld_qkv=24 * HD, ld_out=24 * HD)
    add("rep_hd_over_1024", nq=64, hd=256, ld_qkv=64 * 256, ld_out=64 * 256)
    if wide:
        add("hd_256", hd=256, ld_qkv=NQ * 256, ld_out=NQ * 256)
    if has("max_len") and not paged:  # (a paged launch takes max_pages * page_size and ignores the argument)
        add("max_len_6", max_len=6)
        add("max_len_2", max_len=2)
    add("ld_qkv_short", ld_qkv=NQ * HD - 1)
    add("ld_out_short", ld_out=NQ * HD - 1)
    add("ws_bytes_short", ws_bytes=base["ws_bytes"] - 1)
    add("null_q_hd_96", q=None, hd=96)
    add("hd_96_misaligned_kcache", hd=96, kcache=PTR + 8)
    add("ld_out_short_misaligned_out", ld_out=NQ * HD - 1, out=PTR + 1)
    add("misaligned_q_null_ws", q=PTR + 2, ws=None)
    return out


def table():
    """[(case id, entry point, argument tuple)] — the same list at every call"""
    lib = qp._native.lib()
    rows = []
    for entry, (order, sizer) in ENTRIES.items():
        for flavour, over in _flavours(entry, order):
            base = {p: PTR for p in POINTERS}
            base.update(ld_qkv=NQ * HD, ld_out=NQ * HD, nq=NQ, nkv=NKV, hd=HD, max_len=LEN, scale=0.125, stream=None,
                        rows=130 if entry == "prefill_wide" else 4, S=2, B=3, G=2, ld_table=64, num_pages=100, page_size=16,
                        max_pages=LEN // 16, kv_fmt=0, window=0, softcap=0.0, sinks=None)
            base.update(over)
            base["ws_bytes"] = _ws_bytes(lib, sizer, base)
            assert base["ws_bytes"] > 0, (entry, flavour)  # a null or short workspace is a fault of every launch in the table
            for case, kw in _cases(entry, order, base):
                a = {**base, **kw}
                rows.append(("/".join(x for x in (entry, flavour, case) if x), "qpal_attn_rope_" + entry, tuple(a[n] for n in order)))
    return rows


def run():
    lib = qp._native.lib()
    return {cid: getattr(lib, fn)(*args) for cid, fn, args in table()}


def test_bad_arguments_are_refused_with_the_recorded_codes():
    assert len(ENTRIES) == 18 and all(len(order) == len(qp._native._SIGNATURES["qpal_attn_rope_" + e]) for e, (order, _) in ENTRIES.items())
    got = run()
    launched = {cid: rc for cid, rc in got.items() if rc >= 0}
    assert not launched, f"accepted by the host checks: {launched}"
    want = json.load(open(GOLDEN))
    assert set(got) == set(want)
    diff = {cid: (rc, want[cid]) for cid, rc in got.items() if rc != want[cid]}
    assert not diff, f"{len(diff)} of {len(got)} cases (now, recorded): {dict(list(diff.items())[:20])}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    codes = run()
    assert all(rc < 0 for rc in codes.values()), {c: rc for c, rc in codes.items() if rc >= 0}
    with open(GOLDEN, "w") as f:
        json.dump(codes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(codes)} cases")
