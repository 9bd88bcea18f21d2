"""Python ctypes binding of libcrdt_hip.so (include/crdt_hip.h).

Host plumbing for the tests and bench.py.  The merge itself always runs in the HIP kernels of
libcrdt_hip.so; there is no Python or CPU fallback: if the library is missing, or no device is
present, calls raise.

Mirrors the reference's per-CRDT interface (/root/reference/src/rope.rs:6-33 `Upstream`,
:185-191 `Downstream`) through `HipMerge`, so tests read like the reference's bench loop
(/root/reference/src/main.rs:28-36, :63-69).
"""
from __future__ import annotations

import ctypes as C
import os
from functools import partial as _partial

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# CRDT_HIP_LIB selects another in-tree build (e.g. libcrdt_hip_probe.so: `make probe`)
LIB_PATH = os.path.join(PKG_DIR, os.environ.get("CRDT_HIP_LIB", "libcrdt_hip.so"))

OK = 0
ERRORS = {
    -1: "EINVAL", -2: "ERANGE", -3: "ENOMEM", -4: "EDEVICE", -5: "EBADLOG", -6: "ESPACE",
    -7: "EIO", -8: "ECOMM",
}
STAGES = ["classify", "runs", "sortb", "count", "scan", "place", "link", "walk1", "rank",
          "walk2", "expand", "digest", "doctree", "text", "encode"]


class CrdtHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class View(C.Structure):
    _fields_ = [
        ("n", C.c_uint32),
        ("parent", C.POINTER(C.c_uint32)),
        ("origin_right", C.POINTER(C.c_uint32)),
        ("lamport", C.POINTER(C.c_uint32)),
        ("agent", C.POINTER(C.c_uint16)),
        ("deleted", C.POINTER(C.c_uint8)),
        ("cp", C.POINTER(C.c_uint32)),
        ("side", C.POINTER(C.c_uint8)),  # Fugue (NULL: RGA)
    ]


class Stats(C.Structure):
    _fields_ = [
        ("items", C.c_uint64),
        ("docs", C.c_uint64),
        ("text_bytes", C.c_uint64),
        ("runs", C.c_uint64),
        ("waves", C.c_uint32),
        ("nstages", C.c_uint32),
        ("stage_ns", C.c_uint64 * 16),
        ("stage_launches", C.c_uint32 * 16),
        ("total_ns", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {
            "items": self.items, "docs": self.docs, "text_bytes": self.text_bytes,
            "runs": self.runs, "waves": self.waves, "total_ns": self.total_ns,
            "stage_ns": {STAGES[i]: int(self.stage_ns[i]) for i in range(self.nstages)},
            "stage_launches": {STAGES[i]: int(self.stage_launches[i]) for i in range(self.nstages)},
        }


# (restype, argtypes) of every symbol include/crdt_hip.h declares; lib() sets them, and EXPORTS is
# their names (tests/test_abi.py compares it with the header: a declared symbol has argtypes).
def _signatures() -> dict:
    vp, u32, u64, sz, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int
    P = C.POINTER
    return {
        "crdt_hip_abi_version": (i32, []),
        "crdt_hip_device_count": (i32, [P(i32)]),
        "crdt_hip_init": (i32, [i32, P(vp)]),
        "crdt_hip_destroy": (i32, [vp]),
        "crdt_hip_last_error": (C.c_char_p, [vp]),
        "crdt_hip_set_param": (i32, [vp, C.c_char_p, u64]),
        "crdt_hip_oplog_new": (i32, [P(vp)]),
        "crdt_hip_oplog_set_fugue": (i32, [vp, i32]),
        "crdt_hip_oplog_set_agent": (i32, [vp, C.c_uint16]),
        "crdt_hip_oplog_clone": (i32, [vp, P(vp)]),
        "crdt_hip_oplog_free": (None, [vp]),
        "crdt_hip_oplog_insert": (i32, [vp, sz, C.c_char_p, sz]),
        "crdt_hip_oplog_remove": (i32, [vp, sz, sz]),
        "crdt_hip_oplog_replace": (i32, [vp, sz, sz, C.c_char_p, sz]),
        "crdt_hip_oplog_visible_len": (sz, [vp]),
        "crdt_hip_oplog_get_view": (i32, [vp, P(View)]),
        "crdt_hip_oplog_version": (u64, [vp]),
        "crdt_hip_oplog_encode_from": (i32, [vp, u64, vp, sz, P(sz)]),
        "crdt_hip_oplog_apply_update": (i32, [vp, vp, sz]),
        "crdt_hip_oplog_join": (i32, [vp, P(View), P(u32), P(u32)]),
        "crdt_hip_trace_load": (i32, [C.c_char_p, P(vp)]),
        "crdt_hip_trace_free": (None, [vp]),
        "crdt_hip_trace_len": (sz, [vp]),
        "crdt_hip_trace_txns": (sz, [vp]),
        "crdt_hip_trace_patch": (i32, [vp, sz, P(sz), P(sz), P(C.c_char_p), P(sz)]),
        "crdt_hip_trace_start_content": (i32, [vp, P(vp), P(sz)]),
        "crdt_hip_trace_end_content": (i32, [vp, P(vp), P(sz)]),
        "crdt_hip_trace_chars_to_bytes": (i32, [vp]),
        "crdt_hip_trace_resolve": (i32, [vp, P(vp)]),
        "crdt_hip_trace_resolve_fugue": (i32, [vp, P(vp)]),
        "crdt_hip_trace_resolve_many": (i32, [P(vp), u32, u32, P(vp)]),
        "crdt_hip_trace_save": (i32, [vp, C.c_char_p]),
        "crdt_hip_oplog_save": (i32, [vp, C.c_char_p]),
        "crdt_hip_oplog_load": (i32, [C.c_char_p, P(vp)]),
        "crdt_hip_logfile_open": (i32, [C.c_char_p, P(vp), P(View)]),
        "crdt_hip_logfile_close": (i32, [vp]),
        "crdt_hip_synth_agents": (i32, [u32, u32, u64, P(vp)]),
        "crdt_hip_synth_tree": (i32, [u32, u32, u32, u64, P(vp)]),
        "crdt_hip_synth_tree_visible": (i32, [u32, u32, u64, P(u64)]),
        "crdt_hip_merge": (i32, [vp, P(View), vp, sz, P(sz), P(u64)]),
        "crdt_hip_merge_batch": (i32, [vp, P(View), u32, vp, vp, P(Stats)]),
        "crdt_hip_merge_order": (i32, [vp, P(View), vp]),
        "crdt_hip_batch_create": (i32, [vp, P(View), u32, u32, u32, u64, P(vp)]),
        "crdt_hip_batch_synth_tree": (i32, [vp, u32, u32, u32, u64, P(vp)]),
        "crdt_hip_batch_free": (i32, [vp]),
        "crdt_hip_batch_info": (i32, [vp, P(u64), P(u64), P(u64)]),
        "crdt_hip_batch_merge": (i32, [vp, vp, vp, vp, P(Stats)]),
        "crdt_hip_batch_raw": (i32, [vp, vp, i32]),
        "crdt_hip_replica_new": (i32, [vp, P(View), P(vp)]),
        "crdt_hip_replica_clone": (i32, [vp, vp, P(vp)]),
        "crdt_hip_replica_free": (i32, [vp]),
        "crdt_hip_replica_apply_updates": (i32, [vp, vp, vp, sz, vp, u32]),
        "crdt_hip_updates_upload": (i32, [vp, vp, sz, vp, u32, P(vp)]),
        "crdt_hip_updates_free": (i32, [vp]),
        "crdt_hip_replica_apply_resident": (i32, [vp, vp, vp]),
        "crdt_hip_replica_info": (i32, [vp, P(u64), P(u64), P(u64)]),
        "crdt_hip_replica_join": (i32, [vp, vp, vp, P(u32), P(u32)]),
        "crdt_hip_join_stats": (i32, [vp, P(u64), P(u64), P(u64), P(u64)]),
        "crdt_hip_oplog_state_vector": (i32, [vp, vp, sz, P(sz)]),
        "crdt_hip_oplog_encode_diff": (i32, [vp, vp, sz, vp, sz, P(sz)]),
        "crdt_hip_oplog_apply_diff": (i32, [vp, vp, sz, P(u32), P(u32)]),
        "crdt_hip_replica_state_vector": (i32, [vp, vp, vp, sz, P(sz)]),
        "crdt_hip_replica_encode_diff": (i32, [vp, vp, vp, sz, vp, sz, P(sz)]),
        "crdt_hip_replica_apply_diff": (i32, [vp, vp, vp, sz, P(u32), P(u32)]),
        "crdt_hip_delta_stats": (i32, [vp, P(u64), P(u64), P(u64), P(u64)]),
        "crdt_hip_oplog_mark": (i32, [vp, P(vp)]),
        "crdt_hip_mark_free": (None, [vp]),
        "crdt_hip_oplog_patches_since": (i32, [vp, vp, vp, sz, P(sz), vp, sz, P(sz)]),
        "crdt_hip_replica_mark": (i32, [vp, vp, P(vp)]),
        "crdt_hip_replica_patches_since": (i32, [vp, vp, vp, vp, sz, P(sz), vp, sz, P(sz)]),
        "crdt_hip_patch_stats": (i32, [vp, P(u64), P(u64), P(u64), P(u64)]),
        "crdt_hip_oplog_apply_patches": (i32, [vp, vp, sz, vp, sz, P(u32), P(u32)]),
        "crdt_hip_replica_set_agent": (i32, [vp, C.c_uint16]),
        "crdt_hip_replica_apply_patches": (i32, [vp, vp, vp, sz, vp, sz, P(u32), P(u32)]),
        "crdt_hip_replica_replace": (i32, [vp, vp, sz, sz, C.c_char_p, sz]),
        "crdt_hip_edit_stats": (i32, [vp, P(u64), P(u64), P(u64), P(u64), P(u64)]),
        "crdt_hip_oplog_visible_bytes": (i32, [vp, P(u64)]),
        "crdt_hip_oplog_apply_patches_bytes": (i32, [vp, vp, sz, vp, sz, P(u32), P(u32)]),
        "crdt_hip_oplog_replace_bytes": (i32, [vp, sz, sz, C.c_char_p, sz]),
        "crdt_hip_oplog_patches_since_bytes": (i32, [vp, vp, vp, sz, P(sz), vp, sz, P(sz)]),
        "crdt_hip_replica_apply_patches_bytes": (i32, [vp, vp, vp, sz, vp, sz, P(u32), P(u32)]),
        "crdt_hip_replica_replace_bytes": (i32, [vp, vp, sz, sz, C.c_char_p, sz]),
        "crdt_hip_replica_patches_since_bytes": (i32, [vp, vp, vp, vp, sz, P(sz), vp, sz, P(sz)]),
        "crdt_hip_oplog_anchors_at": (i32, [vp, vp, vp, sz, vp]),
        "crdt_hip_oplog_anchors_at_bytes": (i32, [vp, vp, vp, sz, vp]),
        "crdt_hip_oplog_anchors_resolve": (i32, [vp, vp, sz, vp]),
        "crdt_hip_replica_anchors_at": (i32, [vp, vp, vp, vp, sz, vp]),
        "crdt_hip_replica_anchors_at_bytes": (i32, [vp, vp, vp, vp, sz, vp]),
        "crdt_hip_replica_anchors_resolve": (i32, [vp, vp, vp, sz, vp]),
        "crdt_hip_anchor_stats": (i32, [vp, P(u64), P(u64), P(u64), P(u64)]),
        "crdt_hip_oplog_spans": (i32, [vp, vp, sz, vp, sz, P(sz), vp, sz, P(sz), P(sz)]),
        "crdt_hip_replica_spans": (i32, [vp, vp, vp, sz, vp, sz, P(sz), vp, sz, P(sz), P(sz)]),
        "crdt_hip_format_stats": (i32, [vp, P(u64), P(u64), P(u64), P(u64), P(u64), P(u64)]),
        "crdt_hip_oplog_text_at": (i32, [vp, vp, u64, u64, u32, vp, sz, P(sz), vp]),
        "crdt_hip_replica_text_at": (i32, [vp, vp, vp, u64, u64, u32, vp, sz, P(sz), vp]),
        "crdt_hip_text_stats": (i32, [vp, P(u64), P(u64), P(u64), P(u64)]),
        "crdt_hip_replica_merge": (i32, [vp, vp, vp, sz, P(sz), P(u64)]),
        "crdt_hip_replica_merge_len": (i32, [vp, vp, P(u64), P(u64), P(u64)]),
        "crdt_hip_replica_merge_inc": (i32, [vp, vp, vp, sz, P(sz), P(u64), P(u32)]),
        "crdt_hip_replica_replay": (i32, [vp, vp, vp, P(u64), P(u64), P(u64)]),
        "crdt_hip_merge_len": (i32, [vp, P(View), P(u64), P(u64), P(u64)]),
        "crdt_hip_comm_unique_id": (i32, [vp]),
        "crdt_hip_comm_init": (i32, [vp, i32, i32, vp]),
        "crdt_hip_allgather_u64": (i32, [vp, vp, sz, vp]),
        "crdt_hip_comm_destroy": (i32, [vp]),
        "crdt_hip_xxh64": (u64, [vp, sz, u64]),
        "crdt_hip_tree_digest": (u64, [vp, sz]),
    }


_SIG = _signatures()
EXPORTS = list(_SIG)
_LIB = None


def lib() -> C.CDLL:
    """Load libcrdt_hip.so from the package directory (fails loudly if it is not built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is not built: run `make -C {PKG_DIR}` "
                           "(or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIG.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def _check(rc: int, ctx=None) -> None:
    if rc != OK:
        msg = lib().crdt_hip_last_error(ctx)
        raise CrdtHipError(rc, msg.decode("utf-8", "replace") if msg else "")


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().crdt_hip_device_count(C.byref(n))
    return int(n.value) if rc == OK else 0


def xxh64(data: bytes, seed: int = 0) -> int:
    return int(lib().crdt_hip_xxh64(data, len(data), seed))


def tree_digest(data: bytes) -> int:
    return int(lib().crdt_hip_tree_digest(data, len(data)))


# ------------------------------------------------------------------------------------------------
_NO_SIDE = (C.c_uint8 * 1)(0)  # the side column of an empty Fugue log (never read)


class LogArrays:
    """Anchor op log as numpy SoA (ids 1..n).  Keeps the arrays alive for a View.  `side`
    (optional): 1 = the item is a LEFT child of its parent (Fugue order); None = RGA."""

    FIELDS = ("parent", "origin_right", "lamport", "agent", "deleted", "cp")

    def __init__(self, parent, lamport, agent, deleted, cp, origin_right=None, side=None):
        self.parent = np.ascontiguousarray(parent, dtype=np.uint32)
        n = self.parent.size
        self.lamport = np.ascontiguousarray(lamport, dtype=np.uint32)
        self.agent = np.ascontiguousarray(agent, dtype=np.uint16)
        self.deleted = np.ascontiguousarray(deleted, dtype=np.uint8)
        self.cp = np.ascontiguousarray(cp, dtype=np.uint32)
        self.origin_right = (np.full(n, 0xFFFFFFFF, np.uint32) if origin_right is None
                             else np.ascontiguousarray(origin_right, dtype=np.uint32))
        self.side = None if side is None else np.ascontiguousarray(side, dtype=np.uint8)
        for f in self.FIELDS:
            assert getattr(self, f).size == n, f
        assert self.side is None or self.side.size == n

    @property
    def n(self) -> int:
        return int(self.parent.size)

    def view(self) -> View:
        def p(a, t):
            return a.ctypes.data_as(C.POINTER(t)) if a.size else None
        # a Fugue log stays a Fugue log when empty: a null side means RGA, so an empty side
        # column points at a dummy byte (as the C API's kNoSide does, capi.cpp)
        if self.side is None:
            side = None
        elif self.side.size:
            side = p(self.side, C.c_uint8)
        else:
            side = C.cast(_NO_SIDE, C.POINTER(C.c_uint8))
        return View(self.n, p(self.parent, C.c_uint32), p(self.origin_right, C.c_uint32),
                    p(self.lamport, C.c_uint32), p(self.agent, C.c_uint16),
                    p(self.deleted, C.c_uint8), p(self.cp, C.c_uint32), side)

    def copy(self) -> "LogArrays":
        return LogArrays(self.parent.copy(), self.lamport.copy(), self.agent.copy(),
                         self.deleted.copy(), self.cp.copy(), self.origin_right.copy(),
                         None if self.side is None else self.side.copy())


class SvEntry(C.Structure):
    _fields_ = [("agent", C.c_uint32), ("lamport", C.c_uint32)]


def _sv_pack(sv) -> tuple:
    """[(agent, lamport)] -> (crdt_hip_sv_entry array or None, entries)."""
    sv = list(sv)
    if not sv:
        return None, 0
    arr = (SvEntry * len(sv))()
    for i, (agent, lamport) in enumerate(sv):
        if not (0 <= agent <= 0xFFFFFFFF and 0 <= lamport <= 0xFFFFFFFF):
            raise CrdtHipError(-1, "state vector entry out of range")
        arr[i].agent, arr[i].lamport = agent, lamport
    return arr, len(sv)


def _sv_get(call, ctx=None, guess: int = 0) -> list:
    """call(out, cap, out_n) under the ESPACE convention -> [(agent, lamport)].  `guess`: a first
    capacity to try (a device call scans the log every time)."""
    n = C.c_size_t(0)
    out, cap = ((SvEntry * guess)(), guess) if guess else (None, 0)
    rc = call(out, cap, C.byref(n))
    if rc == -6:
        out = (SvEntry * n.value)()
        rc = call(out, n.value, C.byref(n))
    _check(rc, ctx)
    return [(int(e.agent), int(e.lamport)) for e in out[: n.value]] if n.value else []


def _diff_get(call, ctx=None, guess: int = 0) -> bytes:
    """call(buf, cap, out_len) under the ESPACE convention -> the delta's bytes.  `guess`: a first
    capacity to try (a device encode classifies the log on every call)."""
    need = C.c_size_t(0)
    buf, cap = (C.create_string_buffer(guess), guess) if guess else (None, 0)
    rc = call(buf, cap, C.byref(need))
    if rc == -6:
        buf = C.create_string_buffer(need.value)
        rc = call(buf, need.value, C.byref(need))
    _check(rc, ctx)
    return buf.raw[: need.value]


class Patch(C.Structure):
    """crdt_hip_patch: replace(pos..pos + del, ins[ins_off, ins_off + ins_len))."""
    _fields_ = [("pos", C.c_uint64), ("ins_off", C.c_uint64), ("dele", C.c_uint32),
                ("ins_len", C.c_uint32)]


class Mark:
    """A version of one OpLog or one Replica (crdt_hip_mark), taken by their mark() and passed to
    their patches_since().  It belongs to the object it was taken from (a clone is another owner),
    stays valid across that object's later edits, updates, joins and deltas, and keeps its owner
    alive."""

    def __init__(self, handle, owner):
        self._h = handle
        self.owner = owner

    def close(self) -> None:
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_mark_free(self._h)
            self._h = None

    __del__ = close


def _patches_get(call, ctx=None, guess: tuple = (0, 0)) -> tuple:
    """call(out, cap, out_n, ins, ins_cap, out_ins) under the ESPACE convention -> (the
    crdt_hip_patch array as a structured numpy array, the `ins` bytes).  `guess`: first capacities
    to try (a device call streams the replica's document order every time)."""
    n, nb = C.c_size_t(0), C.c_size_t(0)
    out = np.zeros(guess[0], PATCH_DTYPE)
    ins = np.zeros(guess[1], np.uint8)
    rc = call(out.ctypes.data if out.size else None, out.size, C.byref(n),
              ins.ctypes.data if ins.size else None, ins.size, C.byref(nb))
    if rc == -6:
        out = np.zeros(n.value, PATCH_DTYPE)
        ins = np.zeros(nb.value, np.uint8)
        rc = call(out.ctypes.data if out.size else None, out.size, C.byref(n),
                  ins.ctypes.data if ins.size else None, ins.size, C.byref(nb))
    _check(rc, ctx)
    return out[: n.value], ins[: nb.value].tobytes()


PATCH_DTYPE = np.dtype([("pos", "<u8"), ("ins_off", "<u8"), ("del", "<u4"), ("ins_len", "<u4")])
assert PATCH_DTYPE.itemsize == C.sizeof(Patch) == 24


def _patch_list(raw: tuple) -> list:
    """(crdt_hip_patch array, ins bytes) -> [(pos, del, ins: str)]."""
    arr, ins = raw
    return [(int(p["pos"]), int(p["del"]),
             ins[int(p["ins_off"]): int(p["ins_off"]) + int(p["ins_len"])].decode("utf-8"))
            for p in arr]


def _patches_pack(patches, ins=None) -> tuple:
    """The arguments of an apply_patches call -> (crdt_hip_patch array, `ins` bytes).  `patches`:
    [(pos, del, ins: str)] as patches_since returns them (`ins` None), or a structured array of
    PATCH_DTYPE with its `ins` bytes (the raw form, passed through unchecked)."""
    if ins is not None:
        return np.ascontiguousarray(patches, dtype=PATCH_DTYPE), bytes(ins)
    plist = list(patches)
    arr = np.zeros(len(plist), PATCH_DTYPE)
    parts, off = [], 0
    for k, (pos, dele, text) in enumerate(plist):
        b = text.encode("utf-8")
        arr[k] = (pos, off, dele, len(b))
        parts.append(b)
        off += len(b)
    return arr, b"".join(parts)


# Text windows (crdt_hip.h, "text windows"): a range of the document, now or at a mark.
TEXT_END = 0xFFFFFFFFFFFFFFFF
TEXT_BYTES = 1


class TextInfo(C.Structure):
    """crdt_hip_text_info: the whole version and the window, each in codepoints and UTF-8 bytes."""
    _fields_ = [("len", C.c_uint64), ("len_bytes", C.c_uint64), ("start", C.c_uint64),
                ("start_bytes", C.c_uint64), ("n", C.c_uint64), ("n_bytes", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _text_get(call, mark, start, end, bytes_, ctx=None, guess: int = 0, info_only: bool = False):
    """call(mark handle, start, end, flags, out, cap, out_len, info) under the ESPACE convention ->
    (the window's UTF-8, its info as a dict); info_only: sized with a NULL buffer, ESPACE accepted,
    and only the info is returned.  `guess`: the first capacity to try (a device call streams the
    replica's document order every time)."""
    h = mark._h if mark is not None else None
    e = TEXT_END if end is None else end
    flags = TEXT_BYTES if bytes_ else 0
    n, info = C.c_size_t(0), TextInfo()
    if info_only:
        rc = call(h, start, e, flags, None, 0, C.byref(n), C.byref(info))
        if rc != -6:
            _check(rc, ctx)
        return info.as_dict()
    buf = np.empty(guess, np.uint8)
    rc = call(h, start, e, flags, buf.ctypes.data if buf.size else None, buf.size, C.byref(n),
              C.byref(info))
    if rc == -6:
        buf = np.empty(n.value, np.uint8)
        rc = call(h, start, e, flags, buf.ctypes.data, buf.size, C.byref(n), C.byref(info))
    _check(rc, ctx)
    return buf[: n.value].tobytes(), info.as_dict()


# Anchors (crdt_hip.h, "anchors"): a place in the text named by the identity of the item next to
# the gap, with a bias.
AFTER, BEFORE = 0, 1
LIVE, DEAD, UNKNOWN = 0, 1, 2
EDGE = 0xFFFFFFFFFFFFFFFF


class Anchor(C.Structure):
    """crdt_hip_anchor: 16 plain bytes, shipped to another peer as they are."""
    _fields_ = [("id", C.c_uint64), ("bias", C.c_uint32), ("pad", C.c_uint32)]


class AnchorPos(C.Structure):
    """crdt_hip_anchor_pos: where an anchor lies in the visible document now."""
    _fields_ = [("pos", C.c_uint64), ("pos_bytes", C.c_uint64), ("state", C.c_uint32),
                ("pad", C.c_uint32)]


ANCHOR_DTYPE = np.dtype([("id", "<u8"), ("bias", "<u4"), ("pad", "<u4")])
ANCHOR_POS_DTYPE = np.dtype([("pos", "<u8"), ("pos_bytes", "<u8"), ("state", "<u4"), ("pad", "<u4")])
assert ANCHOR_DTYPE.itemsize == C.sizeof(Anchor) == 16
assert ANCHOR_POS_DTYPE.itemsize == C.sizeof(AnchorPos) == 24


def _anchors_at(call, positions, bias, ctx=None, out=None) -> np.ndarray:
    """call(pos, bias, n, out) -> the crdt_hip_anchor array.  `bias`: a scalar or one per
    position.  `out`: an array to write into (a failed call leaves it untouched)."""
    pos = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(bias, dtype=np.uint8), pos.shape))
    if out is None:
        out = np.zeros(pos.size, ANCHOR_DTYPE)
    assert out.dtype == ANCHOR_DTYPE and out.size == pos.size
    _check(call(pos.ctypes.data if pos.size else None, b.ctypes.data if b.size else None, pos.size,
                out.ctypes.data if out.size else None), ctx)
    return out


def _anchors_pack(anchors) -> np.ndarray:
    """[(id, bias)] or a structured array of ANCHOR_DTYPE (passed through unchecked)."""
    if isinstance(anchors, np.ndarray) and anchors.dtype == ANCHOR_DTYPE:
        return np.ascontiguousarray(anchors)
    alist = list(anchors)
    arr = np.zeros(len(alist), ANCHOR_DTYPE)
    for k, (ident, bias) in enumerate(alist):
        arr[k] = (ident, bias, 0)
    return arr


def _anchors_resolve(call, anchors, ctx=None, out=None) -> np.ndarray:
    """call(anchors, n, out) -> the crdt_hip_anchor_pos array."""
    arr = _anchors_pack(anchors)
    if out is None:
        out = np.zeros(arr.size, ANCHOR_POS_DTYPE)
    assert out.dtype == ANCHOR_POS_DTYPE and out.size == arr.size
    _check(call(arr.ctypes.data if arr.size else None, arr.size,
                out.ctypes.data if out.size else None), ctx)
    return out


def _anchor_list(raw: np.ndarray) -> list:
    return [(int(a["id"]), int(a["bias"])) for a in raw]


def _anchor_pos_list(raw: np.ndarray) -> list:
    return [(int(p["pos"]), int(p["pos_bytes"]), int(p["state"])) for p in raw]


# Formats (crdt_hip.h, "formats"): attribute ranges between two anchors, flattened into spans.
REMOVE = 1
FORMAT_DTYPE = np.dtype([("start", ANCHOR_DTYPE), ("end", ANCHOR_DTYPE), ("op", "<u8"),
                         ("value", "<u8"), ("key", "<u4"), ("flags", "<u4")])
SPAN_DTYPE = np.dtype([("pos", "<u8"), ("pos_bytes", "<u8"), ("len", "<u8"), ("len_bytes", "<u8"),
                       ("attr_off", "<u4"), ("attr_n", "<u4")])
SPAN_ATTR_DTYPE = np.dtype([("value", "<u8"), ("key", "<u4"), ("pad", "<u4")])
assert FORMAT_DTYPE.itemsize == 56 and SPAN_DTYPE.itemsize == 40 and SPAN_ATTR_DTYPE.itemsize == 16


def _formats_pack(formats) -> np.ndarray:
    """[(start, end, key, value, op, flags)] with start and end as (id, bias), or a structured
    array of FORMAT_DTYPE (passed through unchecked)."""
    if isinstance(formats, np.ndarray) and formats.dtype == FORMAT_DTYPE:
        return np.ascontiguousarray(formats)
    flist = list(formats)
    arr = np.zeros(len(flist), FORMAT_DTYPE)
    for k, (start, end, key, value, op, flags) in enumerate(flist):
        arr[k] = ((start[0], start[1], 0), (end[0], end[1], 0), op, value, key, flags)
    return arr


def _spans_get(call, formats, ctx=None, out=None) -> tuple:
    """call(f, n, out, cap, out_n, attrs, attr_cap, out_attrs, pending) under the ESPACE
    convention -> (crdt_hip_span array, crdt_hip_span_attr array, pending).  `out`: a pair of
    arrays to write into, tried once (a failed call leaves them untouched)."""
    arr = _formats_pack(formats)
    n, na, pend = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)

    def once(sp, at):
        return call(arr.ctypes.data if arr.size else None, arr.size,
                    sp.ctypes.data if sp.size else None, sp.size, C.byref(n),
                    at.ctypes.data if at.size else None, at.size, C.byref(na), C.byref(pend))

    if out is not None:
        sp, at = out
        assert sp.dtype == SPAN_DTYPE and at.dtype == SPAN_ATTR_DTYPE
        _check(once(sp, at), ctx)
        return sp[: n.value], at[: na.value], int(pend.value)
    sp, at = np.zeros(0, SPAN_DTYPE), np.zeros(0, SPAN_ATTR_DTYPE)
    rc = once(sp, at)
    if rc == -6:
        sp, at = np.zeros(n.value, SPAN_DTYPE), np.zeros(na.value, SPAN_ATTR_DTYPE)
        rc = once(sp, at)
    _check(rc, ctx)
    return sp[: n.value], at[: na.value], int(pend.value)


def _span_list(raw: tuple) -> tuple:
    """(spans, attrs, pending) -> ([(pos, len, pos_bytes, len_bytes, {key: value})], pending)."""
    sp, at, pend = raw
    return [(int(x["pos"]), int(x["len"]), int(x["pos_bytes"]), int(x["len_bytes"]),
             {int(a["key"]): int(a["value"])
              for a in at[int(x["attr_off"]): int(x["attr_off"]) + int(x["attr_n"])]})
            for x in sp], pend


def _outs(call, n: int, ctx=None, ctype=C.c_uint64) -> tuple:
    """call(p0, ..., p[n-1]) with n out-pointers of `ctype` -> the n values."""
    v = [ctype() for _ in range(n)]
    _check(call(*map(C.byref, v)), ctx)
    return tuple([x.value for x in v])


def _pair(call, ctx=None) -> tuple:
    """call(added, tombstoned) -> (items appended, items tombstoned), the out-pair of every call
    that changes a log or a replica."""
    return _outs(call, 2, ctx, C.c_uint32)


class _Document:
    """What an OpLog and a Replica both are: a document that is synced by deltas, marked, read as
    patches, text windows, anchors and spans, and edited by patches (crdt_hip_oplog_* and
    crdt_hip_replica_* take the same arguments after their handles).  Every docstring says what the
    call does on the log, which is the definition; the replica returns the same thing, byte for
    byte, from HIP kernels over its kept document order, and a call leaves it as a merge_inc would.
    A subclass gives the symbol prefix, the leading handle arguments, the error context and the
    first capacities to try."""

    _PREFIX = ""                # "crdt_hip_oplog_" or "crdt_hip_replica_"
    _GUESS_SV = 0               # state_vector: entries
    _GUESS_DIFF = 0             # encode_diff: bytes
    _GUESS_PATCHES = (0, 0)     # patches_since: patches, inserted bytes
    _GUESS_TEXT = 1 << 12       # text_at: bytes
    _fns: dict                  # this class's C functions by short name, resolved at first use

    def _lead(self) -> tuple:   # the handles every call starts with
        raise NotImplementedError

    _ectx = None                # whose error string a failed call wrote: a context handle, or None

    def _bind(self, name: str):
        """crdt_hip_<kind>_<name> with this document's handles in front."""
        f = self._fns.get(name)
        if f is None:
            f = self._fns[name] = getattr(lib(), self._PREFIX + name)
        return _partial(f, *self._lead())

    # State-vector delta sync (crdt_hip.h, "state-vector delta sync").
    def state_vector(self) -> list:
        """Per agent with an item, the largest lamport among its items: [(agent, lamport)] by agent
        ascending."""
        return _sv_get(self._bind("state_vector"), self._ectx, self._GUESS_SV)

    def encode_diff(self, sv) -> bytes:
        """The delta a peer with state vector `sv` lacks: the items `sv` does not cover, and the
        tombstones of the items it covers as identity ranges.  The document is unchanged."""
        arr, nsv = _sv_pack(sv)
        call = self._bind("encode_diff")
        return _diff_get(lambda *a: call(arr, nsv, *a), self._ectx, self._GUESS_DIFF)

    def apply_diff(self, data: bytes) -> tuple:
        """this document <- this document U delta.  Returns (items appended, items it held that
        became deleted); a rejected delta raises and changes nothing."""
        call = self._bind("apply_diff")
        return _pair(lambda *a: call(data, len(data), *a), self._ectx)

    # Patches since a mark, and text windows (crdt_hip.h, "patches since a mark", "text windows").
    def mark(self) -> Mark:
        """Remember this version of the document (a replica: its tombstone bits packed into a
        device bit plane the mark owns)."""
        h = C.c_void_p()
        _check(self._bind("mark")(C.byref(h)), self._ectx)
        return Mark(h, self)

    def _patches_since(self, name: str, mark: Mark) -> tuple:
        call = self._bind(name)
        return _patches_get(lambda *a: call(mark._h, *a), self._ectx, self._GUESS_PATCHES)

    def patches_since_raw(self, mark: Mark) -> tuple:
        """patches_since as (crdt_hip_patch array as a structured numpy array, `ins` bytes)."""
        return self._patches_since("patches_since", mark)

    def patches_since(self, mark: Mark) -> list:
        """What changed in the document since `mark`, as [(pos, del, ins: str)] ascending in pos:
        applied in that order, each as replace(pos, pos + del, ins), to the text at the mark they
        give the text now."""
        return _patch_list(self.patches_since_raw(mark))

    def patches_since_bytes_raw(self, mark: Mark) -> tuple:
        """patches_since_bytes as (crdt_hip_patch array, `ins` bytes)."""
        return self._patches_since("patches_since_bytes", mark)

    def patches_since_bytes(self, mark: Mark) -> list:
        """patches_since with pos and del in UTF-8 bytes: spliced in order into the UTF-8 of the
        text at the mark they give the UTF-8 now."""
        return _patch_list(self.patches_since_bytes_raw(mark))

    def text_at(self, mark: Mark = None, start: int = 0, end: int = None, bytes: bool = False) -> bytes:
        """The UTF-8 of window [start, end) of the version now (`mark` None) or at `mark`, in
        codepoints or, with `bytes`, in UTF-8 bytes; `end` None is the version's end.  The text at
        a mark is byte for byte what the document held when the mark was taken.  (A replica writes
        only the tiles of its document order that the window overlaps.)"""
        return _text_get(self._bind("text_at"), mark, start, end, bytes, self._ectx,
                         guess=self._GUESS_TEXT)[0]

    def text_info(self, mark: Mark = None, start: int = 0, end: int = None, bytes: bool = False) -> dict:
        """crdt_hip_text_info of that window alone: len, len_bytes, start, start_bytes, n, n_bytes
        (a position translation between codepoints and bytes; a replica: the count and scan, no
        write pass)."""
        return _text_get(self._bind("text_at"), mark, start, end, bytes, self._ectx, info_only=True)

    # Local edits, in codepoints and in UTF-8 bytes (crdt_hip.h, "local edits", "byte offsets").  A
    # byte call on a log walks the whole document; a replica translates the boundaries to codepoint
    # ranks in HIP kernels against its kept order, and keeps no text on the host.
    def _apply_patches(self, name: str, patches, ins) -> tuple:
        arr, text = _patches_pack(patches, ins)
        call = self._bind(name)
        return _pair(lambda *a: call(arr.ctypes.data if arr.size else None, arr.size, text, len(text),
                                     *a), self._ectx)

    def apply_patches(self, patches, ins=None) -> tuple:
        """Local edits as a set of positional patches in the patches_since convention:
        [(pos, del, ins: str)] ascending and non-touching, each applied as
        replace(pos, pos + del, ins) to the document as the earlier ones left it (a replica: the
        same resulting log, slot for slot).  Returns (items appended, items deleted); a rejected
        call raises and changes nothing."""
        return self._apply_patches("apply_patches", patches, ins)

    def apply_patches_bytes(self, patches, ins=None) -> tuple:
        """apply_patches with pos and del in UTF-8 bytes: the log apply_patches gives for the
        patches translated through the text before the call.  A boundary inside a codepoint raises
        EINVAL.  Returns (items appended, items deleted)."""
        return self._apply_patches("apply_patches_bytes", patches, ins)

    def replace_bytes(self, start: int, end: int, text: str) -> None:
        """Upstream::replace in byte offsets: one patch."""
        b = text.encode("utf-8")
        _check(self._bind("replace_bytes")(start, end, b, len(b)), self._ectx)

    def insert_bytes(self, pos: int, text: str) -> None:
        self.replace_bytes(pos, pos, text)

    def remove_bytes(self, start: int, end: int) -> None:
        if end < start:
            raise CrdtHipError(-2, "remove range out of range")
        self.replace_bytes(start, end, "")

    # Anchors and formats (crdt_hip.h, "anchors", "formats").  A call on a log walks the whole
    # document; a call on a replica changes no log contents.
    def anchors_at_raw(self, positions, bias=AFTER, out=None) -> np.ndarray:
        return _anchors_at(self._bind("anchors_at"), positions, bias, self._ectx, out)

    def anchors_at_bytes_raw(self, positions, bias=AFTER, out=None) -> np.ndarray:
        return _anchors_at(self._bind("anchors_at_bytes"), positions, bias, self._ectx, out)

    def resolve_anchors_raw(self, anchors, out=None) -> np.ndarray:
        return _anchors_resolve(self._bind("anchors_resolve"), anchors, self._ectx, out)

    def anchors_at(self, positions, bias=AFTER) -> list:
        """Gap positions 0..len of the visible document (codepoints) -> [(id, bias)]: AFTER names
        the item before the gap, BEFORE the one after it, EDGE the document's start or end.
        `bias`: a scalar or one per position."""
        return _anchor_list(self.anchors_at_raw(positions, bias))

    def anchors_at_bytes(self, positions, bias=AFTER) -> list:
        """anchors_at with positions in UTF-8 bytes; one inside a codepoint raises EINVAL."""
        return _anchor_list(self.anchors_at_bytes_raw(positions, bias))

    def resolve_anchors(self, anchors) -> list:
        """[(id, bias)], made here or on any peer -> [(pos, pos_bytes, state)] in the visible
        document now; state LIVE, DEAD (the item is tombstoned: the anchor lies where it was) or
        UNKNOWN (the document does not hold the item yet)."""
        return _anchor_pos_list(self.resolve_anchors_raw(anchors))

    def spans_raw(self, formats, out=None) -> tuple:
        return _spans_get(self._bind("spans"), formats, self._ectx, out)

    def spans(self, formats) -> tuple:
        """Attribute ranges [(start, end, key, value, op, flags)] (start, end: anchors (id, bias);
        flags 0 or REMOVE) -> ([(pos, len, pos_bytes, len_bytes, {key: value})], pending): the
        non-overlapping spans of the visible document, per key the covering format with the largest
        op winning, and the formats whose anchors this document cannot place yet."""
        return _span_list(self.spans_raw(formats))


class OpLog(_Document):
    """Host-side resolver (positional patches -> anchor op log), crdt_hip_oplog_*."""

    _PREFIX = "crdt_hip_oplog_"
    _fns: dict = {}

    def _lead(self) -> tuple:
        return (self._h,)

    def __init__(self, handle=None, fugue: bool = False, agent: int = 0):
        if handle is None:
            h = C.c_void_p()
            _check(lib().crdt_hip_oplog_new(C.byref(h)))
            handle = h
            if fugue:
                _check(lib().crdt_hip_oplog_set_fugue(h, 1))
        self._h = handle
        if agent:
            _check(lib().crdt_hip_oplog_set_agent(self._h, agent))

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_oplog_free(self._h)
            self._h = None

    def clone(self) -> "OpLog":
        h = C.c_void_p()
        _check(lib().crdt_hip_oplog_clone(self._h, C.byref(h)))
        return OpLog(h)

    def set_agent(self, agent: int) -> None:
        """The agent id of this log's later local inserts: a fork sets its own on its clone, so
        that (lamport, agent) identifies its items (crdt_hip_oplog_set_agent)."""
        _check(lib().crdt_hip_oplog_set_agent(self._h, agent))

    def join(self, other) -> tuple:
        """State-based merge (crdt_hip_oplog_join): this log <- this log U `other` (an OpLog,
        LogArrays or LogFile) by item identity (lamport, agent).  Returns (items appended, items
        this log held that the join tombstoned); a rejected join raises and changes nothing.
        Two RGA logs or two Fugue logs: a Fugue item's side is an attribute that comes along, not
        part of its identity.  The kind is the presence of the side column (OpLog(fugue=True),
        LogArrays with `side`), never its contents; a mixed pair raises EINVAL."""
        v, keep = _as_view(other)
        return _pair(lambda *a: lib().crdt_hip_oplog_join(self._h, C.byref(v), *a))

    def insert(self, pos: int, text: str) -> None:
        b = text.encode("utf-8")
        _check(lib().crdt_hip_oplog_insert(self._h, pos, b, len(b)))

    def remove(self, start: int, end: int) -> None:
        _check(lib().crdt_hip_oplog_remove(self._h, start, end))

    def replace(self, start: int, end: int, text: str) -> None:
        b = text.encode("utf-8")
        _check(lib().crdt_hip_oplog_replace(self._h, start, end, b, len(b)))

    def visible_len(self) -> int:
        return int(lib().crdt_hip_oplog_visible_len(self._h))

    def view(self) -> View:
        v = View()
        _check(lib().crdt_hip_oplog_get_view(self._h, C.byref(v)))
        return v

    def arrays(self) -> LogArrays:
        v = self.view()
        n = v.n

        def arr(ptr, dt):
            if n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)
        side = None
        if v.side:
            side = arr(v.side, np.uint8)
        return LogArrays(arr(v.parent, np.uint32), arr(v.lamport, np.uint32),
                         arr(v.agent, np.uint16), arr(v.deleted, np.uint8),
                         arr(v.cp, np.uint32), arr(v.origin_right, np.uint32), side)

    def version(self) -> int:
        return int(lib().crdt_hip_oplog_version(self._h))

    def encode_from(self, version: int) -> bytes:
        return _diff_get(lambda *a: lib().crdt_hip_oplog_encode_from(self._h, version, *a))

    def apply_update(self, update: bytes) -> None:
        _check(lib().crdt_hip_oplog_apply_update(self._h, update, len(update)))

    def visible_bytes(self) -> int:
        """UTF-8 bytes of the visible document (crdt_hip_oplog_visible_bytes)."""
        return _outs(lambda *a: lib().crdt_hip_oplog_visible_bytes(self._h, *a), 1)[0]

    def save(self, path: str) -> None:
        """Op-log file (crdt_hip_oplog_save): 64-byte-aligned SoA arrays."""
        _check(lib().crdt_hip_oplog_save(self._h, path.encode()))

    @staticmethod
    def load(path: str) -> "OpLog":
        h = C.c_void_p()
        _check(lib().crdt_hip_oplog_load(path.encode(), C.byref(h)))
        return OpLog(h)

    @staticmethod
    def synth_agents(n_items: int, agents: int, seed: int) -> "OpLog":
        h = C.c_void_p()
        _check(lib().crdt_hip_synth_agents(n_items, agents, seed, C.byref(h)))
        return OpLog(h)

    @staticmethod
    def synth_tree(n_items: int, p_chain_pct: int, del_pct: int, seed: int) -> "OpLog":
        h = C.c_void_p()
        _check(lib().crdt_hip_synth_tree(n_items, p_chain_pct, del_pct, seed, C.byref(h)))
        return OpLog(h)


class Trace:
    """josephg trace loaded by the native loader (crdt_hip_trace_*)."""

    def __init__(self, path: str):
        h = C.c_void_p()
        _check(lib().crdt_hip_trace_load(path.encode(), C.byref(h)))
        self._h = h
        self.path = path

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_trace_free(self._h)
            self._h = None

    def __len__(self) -> int:
        return int(lib().crdt_hip_trace_len(self._h))

    @property
    def txns(self) -> int:
        return int(lib().crdt_hip_trace_txns(self._h))

    def patch(self, i: int):
        pos, dele, n = C.c_size_t(), C.c_size_t(), C.c_size_t()
        ins = C.c_char_p()
        _check(lib().crdt_hip_trace_patch(self._h, i, C.byref(pos), C.byref(dele),
                                          C.byref(ins), C.byref(n)))
        return int(pos.value), int(dele.value), C.string_at(ins, n.value).decode("utf-8")

    def _content(self, fn) -> str:
        p, n = C.c_void_p(), C.c_size_t()
        _check(fn(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value).decode("utf-8") if n.value else ""

    @property
    def start_content(self) -> str:
        return self._content(lib().crdt_hip_trace_start_content)

    @property
    def end_content(self) -> str:
        return self._content(lib().crdt_hip_trace_end_content)

    def chars_to_bytes(self) -> None:
        _check(lib().crdt_hip_trace_chars_to_bytes(self._h))

    def resolve(self, fugue: bool = False) -> OpLog:
        """Positional patches -> anchor op log (RGA anchors; `fugue`: Fugue anchors)."""
        h = C.c_void_p()
        fn = lib().crdt_hip_trace_resolve_fugue if fugue else lib().crdt_hip_trace_resolve
        _check(fn(self._h, C.byref(h)))
        return OpLog(h)

    @staticmethod
    def resolve_many(traces, threads: int = 0):
        """resolve() of every trace, on up to `threads` host threads (0: one per trace)."""
        n = len(traces)
        ins = (C.c_void_p * n)(*[t._h for t in traces])
        outs = (C.c_void_p * n)()
        _check(lib().crdt_hip_trace_resolve_many(ins, n, threads, outs))
        return [OpLog(C.c_void_p(outs[i])) for i in range(n)]

    def save(self, path: str) -> None:
        """Trace cache (crdt_hip_trace_save); Trace(path) reads it back without gunzip + JSON."""
        _check(lib().crdt_hip_trace_save(self._h, path.encode()))


class LogFile:
    """An op-log file mapped read-only (crdt_hip_logfile_open): view() points into the mapping,
    so it can be merged, batched or uploaded without a host copy."""

    def __init__(self, path: str):
        h = C.c_void_p()
        self._v = View()
        _check(lib().crdt_hip_logfile_open(path.encode(), C.byref(h), C.byref(self._v)))
        self._h = h
        self.path = path

    def close(self) -> None:
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_logfile_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def view(self) -> View:
        if not self._h:
            raise ValueError("log file is closed")
        return self._v

    def arrays(self) -> LogArrays:
        v, n = self.view(), self._v.n

        def arr(ptr, dt):
            if n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)
        return LogArrays(arr(v.parent, np.uint32), arr(v.lamport, np.uint32),
                         arr(v.agent, np.uint16), arr(v.deleted, np.uint8),
                         arr(v.cp, np.uint32), arr(v.origin_right, np.uint32),
                         arr(v.side, np.uint8) if v.side else None)


def _as_view(log) -> tuple:
    """(View, keepalive) for an OpLog or LogArrays."""
    if isinstance(log, OpLog):
        return log.view(), log
    if isinstance(log, (LogArrays, LogFile)):
        return log.view(), log
    raise TypeError(type(log))


class Context:
    """One HIP device + its merge engine (crdt_hip_init)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(lib().crdt_hip_init(device, C.byref(h)))
        self._h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_destroy(self._h)
            self._h = None

    __del__ = close

    def set_param(self, key: str, value: int) -> None:
        _check(lib().crdt_hip_set_param(self._h, key.encode(), value), self._h)

    def _stats(self, name: str, fields: tuple) -> dict:
        """crdt_hip_<name>_stats: what this context's last device call of that kind observed."""
        fn = getattr(lib(), f"crdt_hip_{name}_stats")
        return dict(zip(fields, _outs(lambda *a: fn(self._h, *a), len(fields), self._h)))

    def join_stats(self) -> dict:
        """What this context's last Replica.join observed (crdt_hip_join_stats)."""
        return self._stats("join", ("prefix_slots", "table_slots", "table_capacity", "device_ns"))

    def delta_stats(self) -> dict:
        """What this context's last Replica.encode_diff or apply_diff observed
        (crdt_hip_delta_stats)."""
        return self._stats("delta", ("items", "ranges", "table_slots", "device_ns"))

    def patch_stats(self) -> dict:
        """What this context's last Replica.patches_since observed (crdt_hip_patch_stats)."""
        return self._stats("patch", ("patches", "ins_bytes", "ranks", "device_ns"))

    def edit_stats(self) -> dict:
        """What this context's last Replica.apply_patches (or replace, insert, remove) observed
        (crdt_hip_edit_stats)."""
        return self._stats("edit", ("patches", "items", "tombstones", "ranks", "device_ns"))

    def anchor_stats(self) -> dict:
        """What this context's last Replica.anchors_at or resolve_anchors observed
        (crdt_hip_anchor_stats)."""
        return self._stats("anchor", ("anchors", "unknown", "ranks", "device_ns"))

    def text_stats(self) -> dict:
        """What this context's last Replica.text_at or text_info observed (crdt_hip_text_stats)."""
        return self._stats("text", ("ranks", "tiles_written", "bytes", "device_ns"))

    def format_stats(self) -> dict:
        """What this context's last Replica.spans observed (crdt_hip_format_stats)."""
        return self._stats("format", ("formats", "pending", "segments", "spans", "ranks", "device_ns"))

    def merge(self, log) -> tuple:
        """Merged document: (utf8 bytes, tree digest)."""
        v, keep = _as_view(log)
        cap = 4 * v.n + 16
        buf = np.empty(cap, np.uint8)  # (not zeroed: the engine writes the n bytes returned)
        n, dig = C.c_size_t(), C.c_uint64()
        _check(lib().crdt_hip_merge(self._h, C.byref(v), buf.ctypes.data, cap, C.byref(n),
                                    C.byref(dig)), self._h)
        del keep
        return buf[: n.value].tobytes(), int(dig.value)

    def merge_digest(self, log) -> tuple:
        v, keep = _as_view(log)
        n, dig = C.c_size_t(), C.c_uint64()
        _check(lib().crdt_hip_merge(self._h, C.byref(v), None, 0, C.byref(n), C.byref(dig)),
               self._h)
        return int(n.value), int(dig.value)

    def merge_len(self, log) -> tuple:
        """Upstream::len on the device: (codepoints, UTF-8 bytes, tree digest) of the merged
        document, without copying the text back (crdt_hip_merge_len)."""
        v, keep = _as_view(log)
        return _outs(lambda *a: lib().crdt_hip_merge_len(self._h, C.byref(v), *a), 3, self._h)

    def merge_batch(self, logs: list, stats: bool = False):
        views = []
        keep = []
        for lg in logs:
            v, k = _as_view(lg)
            views.append(v)
            keep.append(k)
        arr = (View * len(views))(*views)
        dig = np.zeros(len(views), np.uint64)
        lens = np.zeros(len(views), np.uint64)
        st = Stats()
        _check(lib().crdt_hip_merge_batch(self._h, arr, len(views), dig.ctypes.data,
                                          lens.ctypes.data, C.byref(st)), self._h)
        return (dig, lens, st.as_dict()) if stats else (dig, lens)

    def merge_order(self, log) -> np.ndarray:
        v, keep = _as_view(log)
        out = np.zeros(max(v.n, 1), np.uint32)
        _check(lib().crdt_hip_merge_order(self._h, C.byref(v), out.ctypes.data), self._h)
        return out[: v.n]

    def batch(self, bases: list, replicas: int, relabel: int = 0, seed: int = 0) -> "Batch":
        return Batch(self, bases, replicas, relabel, seed)

    # RCCL
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().crdt_hip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes) -> None:
        _check(lib().crdt_hip_comm_init(self._h, nranks, rank, uid), self._h)

    def allgather_u64(self, values: np.ndarray, nranks: int) -> np.ndarray:
        v = np.ascontiguousarray(values, dtype=np.uint64)
        out = np.zeros(v.size * nranks, np.uint64)
        _check(lib().crdt_hip_allgather_u64(self._h, v.ctypes.data, v.size, out.ctypes.data),
               self._h)
        return out


def synth_tree_visible(n_items: int, del_pct: int, seed: int) -> int:
    """Visible items (= merged bytes) of OpLog.synth_tree(n_items, *, del_pct, seed)."""
    out = C.c_uint64()
    _check(lib().crdt_hip_synth_tree_visible(n_items, del_pct, seed, C.byref(out)))
    return int(out.value)


class Batch:
    """Device-resident replica batch (crdt_hip_batch_*)."""

    RELABEL = {"none": 0, "rotate": 1, "shuffle": 2}

    def __init__(self, ctx: Context, bases: list, replicas: int, relabel=0, seed: int = 0,
                 _handle=None):
        if _handle is not None:
            h = _handle
        else:
            if isinstance(relabel, str):
                relabel = self.RELABEL[relabel]
            views = []
            keep = []
            for b in bases:
                v, k = _as_view(b)
                views.append(v)
                keep.append(k)
            arr = (View * len(views))(*views)
            h = C.c_void_p()
            _check(lib().crdt_hip_batch_create(ctx._h, arr, len(views), replicas, relabel, seed,
                                               C.byref(h)), ctx._h)
        self._h = h
        self.ctx = ctx
        self.docs, self.items, self.device_bytes = _outs(
            lambda *a: lib().crdt_hip_batch_info(h, *a), 3)

    @classmethod
    def synth_tree(cls, ctx: Context, n_items: int, p_chain_pct: int, del_pct: int,
                   seed: int) -> "Batch":
        """One config-5 document generated on the device (= OpLog.synth_tree, no host copy)."""
        h = C.c_void_p()
        _check(lib().crdt_hip_batch_synth_tree(ctx._h, n_items, p_chain_pct, del_pct, seed,
                                               C.byref(h)), ctx._h)
        return cls(ctx, [], 0, _handle=h)

    def close(self) -> None:
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_batch_free(self._h)
            self._h = None

    __del__ = close

    def merge(self):
        dig = np.zeros(self.docs, np.uint64)
        lens = np.zeros(self.docs, np.uint64)
        st = Stats()
        _check(lib().crdt_hip_batch_merge(self.ctx._h, self._h, dig.ctypes.data,
                                          lens.ctypes.data, C.byref(st)), self.ctx._h)
        return dig, lens, st.as_dict()

    def set_raw(self, on: bool = True) -> None:
        """Raw SoA mode (crdt_hip_batch_raw): every merge derives its input encoding on the device
        from reference-shaped columns (lamport, agent, deleted, codepoint beside the parents)."""
        _check(lib().crdt_hip_batch_raw(self.ctx._h, self._h, int(bool(on))), self.ctx._h)


def pack_updates(updates) -> tuple:
    """Concatenate encoded updates: (bytes as np.uint8, n + 1 byte offsets as np.uint64)."""
    lens = np.fromiter((len(u) for u in updates), np.uint64, count=len(updates))
    offsets = np.zeros(len(updates) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    buf = np.frombuffer(b"".join(updates), np.uint8) if updates else np.zeros(0, np.uint8)
    return buf, offsets


class UpdateBatch:
    """Encoded updates uploaded to HBM once (crdt_hip_updates_*), applied to any replica of the
    context by Replica.apply_resident: Downstream's update vector (main.rs:58) kept on the device."""

    def __init__(self, ctx: "Context", buf: np.ndarray, offsets: np.ndarray):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().crdt_hip_updates_upload(ctx._h, buf.ctypes.data if buf.size else None,
                                             buf.size, offsets.ctypes.data,
                                             max(0, offsets.size - 1), C.byref(h)), ctx._h)
        self._h = h
        self.ctx = ctx
        self.n = max(0, offsets.size - 1)

    def close(self) -> None:
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_updates_free(self._h)
            self._h = None

    __del__ = close


class Replica(_Document):
    """Device-resident replica (crdt_hip_replica_*): Downstream on the device.

    Updates (OpLog.encode_from's wire format) are decoded by the HIP kernels straight into the
    replica's HBM slot arrays, a whole batch per call, and the replica is merged where it lies.
    """

    _PREFIX = "crdt_hip_replica_"
    _fns: dict = {}
    # (a device call scans or streams the whole replica every time: room for most answers at once)
    _GUESS_SV, _GUESS_DIFF, _GUESS_PATCHES, _GUESS_TEXT = 256, 1 << 20, (4096, 1 << 16), 1 << 16

    def _lead(self) -> tuple:
        return (self.ctx._h, self._h)

    @property
    def _ectx(self):
        return self.ctx._h

    def __init__(self, ctx: Context, init=None, _handle=None):
        if _handle is None:
            h = C.c_void_p()
            if init is None:
                rc = lib().crdt_hip_replica_new(ctx._h, None, C.byref(h))
            else:
                v, keep = _as_view(init)
                rc = lib().crdt_hip_replica_new(ctx._h, C.byref(v), C.byref(h))
            _check(rc, ctx._h)
            _handle = h
        self._h = _handle
        self.ctx = ctx

    def close(self) -> None:
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.crdt_hip_replica_free(self._h)
            self._h = None

    __del__ = close

    def clone(self) -> "Replica":
        h = C.c_void_p()
        _check(lib().crdt_hip_replica_clone(self.ctx._h, self._h, C.byref(h)), self.ctx._h)
        return Replica(self.ctx, _handle=h)

    def apply_packed(self, buf: np.ndarray, offsets: np.ndarray) -> None:
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if n <= 0:
            return
        _check(lib().crdt_hip_replica_apply_updates(
            self.ctx._h, self._h, buf.ctypes.data if buf.size else None, buf.size,
            offsets.ctypes.data, n), self.ctx._h)

    def apply_updates(self, updates) -> None:
        self.apply_packed(*pack_updates(list(updates)))

    def apply_resident(self, batch: "UpdateBatch") -> None:
        """Apply a batch already in HBM (crdt_hip_replica_apply_resident): no PCIe transfer."""
        _check(lib().crdt_hip_replica_apply_resident(self.ctx._h, self._h, batch._h), self.ctx._h)

    def join(self, other: "Replica") -> tuple:
        """State-based merge on the device (crdt_hip_replica_join): this replica <- this replica U
        `other` by item identity (lamport, agent); `other` is unchanged.  Returns (items appended,
        items this replica held that the join tombstoned); a rejected join raises and changes
        nothing.  Two RGA replicas or two Fugue replicas (made from a Fugue log or view, empty or
        not): a Fugue item's identity is its key without the side bit, and an appended item keeps
        its side; a mixed pair raises EINVAL."""
        return _pair(lambda *a: lib().crdt_hip_replica_join(self.ctx._h, self._h, other._h, *a),
                     self.ctx._h)

    def set_agent(self, agent: int) -> None:
        """The agent id of this replica's later local edits (crdt_hip_replica_set_agent; default
        0, kept by a clone)."""
        _check(lib().crdt_hip_replica_set_agent(self._h, agent))

    def replace(self, start: int, end: int, text: str) -> None:
        """Upstream::replace on the device (crdt_hip_replica_replace): one patch."""
        b = text.encode("utf-8")
        _check(lib().crdt_hip_replica_replace(self.ctx._h, self._h, start, end, b, len(b)),
               self.ctx._h)

    def insert(self, pos: int, text: str) -> None:
        self.replace(pos, pos, text)

    def remove(self, start: int, end: int) -> None:
        if end < start:
            raise CrdtHipError(-2, "remove range out of range")
        self.replace(start, end, "")

    def info(self) -> tuple:
        """(items, visible codepoints, visible UTF-8 bytes)."""
        return _outs(lambda *a: lib().crdt_hip_replica_info(self._h, *a), 3)

    def merge(self) -> tuple:
        """Merged document: (utf8 bytes, tree digest)."""
        cap = self.info()[2] + 16
        buf = C.create_string_buffer(cap)
        n, dig = C.c_size_t(), C.c_uint64()
        _check(lib().crdt_hip_replica_merge(self.ctx._h, self._h, buf, cap, C.byref(n),
                                            C.byref(dig)), self.ctx._h)
        return buf.raw[: n.value], int(dig.value)

    def merge_digest(self) -> tuple:
        n, dig = C.c_size_t(), C.c_uint64()
        _check(lib().crdt_hip_replica_merge(self.ctx._h, self._h, None, 0, C.byref(n),
                                            C.byref(dig)), self.ctx._h)
        return int(n.value), int(dig.value)

    def merge_inc(self, text: bool = False) -> tuple:
        """Incremental len() (crdt_hip_replica_merge_inc): (codepoints, UTF-8 bytes, path, text or
        None); path 1 = only the items appended since the previous call were ranked, 0 = a full
        merge (first call, concurrent update, > 4096 new items, Fugue)."""
        cap = self.info()[2] + 16 if text else 0
        buf = C.create_string_buffer(cap) if text else None
        n, c, p = C.c_size_t(), C.c_uint64(), C.c_uint32()
        _check(lib().crdt_hip_replica_merge_inc(self.ctx._h, self._h, buf, cap, C.byref(n),
                                                C.byref(c), C.byref(p)), self.ctx._h)
        return int(c.value), int(n.value), int(p.value), (buf.raw[: n.value] if text else None)

    def replay(self, batch: "UpdateBatch") -> tuple:
        """The downstream closure (main.rs:63-69) in one device call: a copy of this replica
        receives the whole resident batch and is merged; returns (codepoints, UTF-8 bytes, tree
        digest) and leaves this replica unchanged (crdt_hip_replica_replay)."""
        return _outs(lambda *a: lib().crdt_hip_replica_replay(self.ctx._h, self._h, batch._h, *a), 3,
                     self.ctx._h)

    def merge_len(self) -> tuple:
        """(codepoints, UTF-8 bytes, tree digest) of the merged document; the codepoints are
        counted on the device from the merged bytes (crdt_hip_replica_merge_len)."""
        return _outs(lambda *a: lib().crdt_hip_replica_merge_len(self.ctx._h, self._h, *a), 3,
                     self.ctx._h)


class _Adapter:
    """What HipMerge, HipDownstream and HipDownstreamBytes share: the reference's `Upstream` edits
    (rope.rs:6-33), sync, marks, text windows, anchors and formats, all on _rt_peer(), the document
    the adapter holds (an OpLog; for the device adapters the Replica, queued updates decoded first).
    Positions, patches and lengths are in the adapter's unit, codepoints or, with
    EDITS_USE_BYTE_OFFSETS, UTF-8 bytes (translated on the device: crdt_hip.h, "byte offsets").

    Formats (crdt_hip.h, "formats"): the adapter keeps its format ops in a dict by op, makes their
    anchors where its document lies, and paints spans in its own unit.  Formats travel beside the
    text, never in it: sync_formats_from is the union of two dicts."""

    EDITS_USE_BYTE_OFFSETS = False
    START, END = 1, 2  # `expand` bits: text typed at that edge of the range joins it
    agent = 0          # the low 16 bits of this peer's format ops (set_agent)

    def _rt_peer(self):  # what holds the document: an OpLog or a Replica, up to date
        raise NotImplementedError

    # Upstream (rope.rs:6-33)
    def insert(self, at: int, text: str) -> None:
        doc = self._rt_peer()
        (doc.insert_bytes if self.EDITS_USE_BYTE_OFFSETS else doc.insert)(at, text)

    def remove(self, start: int, end: int) -> None:
        doc = self._rt_peer()
        (doc.remove_bytes if self.EDITS_USE_BYTE_OFFSETS else doc.remove)(start, end)

    def replace(self, start: int, end: int, text: str) -> None:
        doc = self._rt_peer()
        (doc.replace_bytes if self.EDITS_USE_BYTE_OFFSETS else doc.replace)(start, end, text)

    def merge_from(self, other) -> tuple:
        """`Downstream for Automerge`'s apply_update(&mut self, other: &Self) = doc.merge(other)
        (rope.rs:234-236): take every op of a divergent replica (join; both documents RGA or both
        Fugue)."""
        return self._rt_peer().join(other._rt_peer())

    def sync_from(self, other) -> tuple:
        """The Yrs Downstream (rope.rs:252-255): state_vector(), the other's encode_diff against
        it, apply_update.  Takes what this document lacks of a divergent replica without moving the
        other's whole log.  Returns (items appended, items tombstoned, delta bytes)."""
        doc = self._rt_peer()
        delta = other._rt_peer().encode_diff(doc.state_vector())
        return doc.apply_diff(delta) + (len(delta),)

    def mark(self) -> Mark:
        """Remember this version of the document."""
        return self._rt_peer().mark()

    def patches_since(self, mark: Mark) -> list:
        """What changed since `mark` as [(pos, del, ins)], the reference's TestPatch applied as
        Upstream::replace (rope.rs:21-32): what an editor that keeps a text buffer beside this
        adapter applies to it after a remote change."""
        doc = self._rt_peer()
        return (doc.patches_since_bytes if self.EDITS_USE_BYTE_OFFSETS else doc.patches_since)(mark)

    def sync_patches(self, other) -> list:
        """mark, sync_from(other), patches_since: the other's changes as positional edits."""
        m = self.mark()
        try:
            self.sync_from(other)
            return self.patches_since(m)
        finally:
            m.close()

    def text_range(self, start: int, end: int = None) -> str:
        """Window [start, end) of the document now: what an editor paints (a device adapter gets
        only the window back)."""
        return self.text_at(None, start, end)

    def text_at(self, mark: Mark, start: int = 0, end: int = None) -> str:
        """The document as of `mark`, or window [start, end) of it: history without a saved copy of
        the text."""
        return self._rt_peer().text_at(mark, start, end, self.EDITS_USE_BYTE_OFFSETS).decode("utf-8")

    def _rt_anchors(self, positions, bias) -> list:
        doc = self._rt_peer()
        return (doc.anchors_at_bytes if self.EDITS_USE_BYTE_OFFSETS else doc.anchors_at)(positions, bias)

    def anchor_at(self, pos: int, bias: int = AFTER) -> tuple:
        """A cursor at gap `pos` as (id, bias): a place that survives every later edit and sync and
        means the same on every peer."""
        return self._rt_anchors([pos], bias)[0]

    def resolve_many(self, anchors) -> list:
        """Where each anchor lies now; None for one whose item this document does not hold yet."""
        unit = 1 if self.EDITS_USE_BYTE_OFFSETS else 0
        return [None if p[2] == UNKNOWN else p[unit] for p in self._rt_peer().resolve_anchors(anchors)]

    def resolve(self, anchor: tuple):
        return self.resolve_many([anchor])[0]

    def set_agent(self, agent: int) -> None:
        """This peer's agent id, for its later text edits and its later format ops alike."""
        self._rt_peer().set_agent(agent)
        self.agent = agent

    @property
    def formats(self) -> dict:
        """{op: (start, end, key, value, flags)}, start and end as anchors (id, bias)."""
        if "_formats" not in self.__dict__:
            self._formats = {}
        return self._formats

    def _rt_add(self, start: int, end: int, key: int, value: int, flags: int, expand: int) -> int:
        peer = self._rt_peer()
        a = self._rt_anchors([start, end], [AFTER if expand & self.START else BEFORE,
                                            BEFORE if expand & self.END else AFTER])
        clock = max(max((lam for _, lam in peer.state_vector()), default=0),
                    self.__dict__.get("_format_clock", 0)) + 1
        self._format_clock = clock
        op = (clock << 16) | self.agent
        self.formats[op] = (a[0], a[1], key, value, flags)
        return op

    def format(self, start: int, end: int, key: int, value: int, expand: int = 0) -> int:
        """Give the text between the gaps `start` and `end` the attribute (key, value); returns the
        op.  `expand`: START | END, the edges at which text typed later joins the range."""
        return self._rt_add(start, end, key, value, 0, expand)

    def unformat(self, start: int, end: int, key: int, expand: int = 0) -> int:
        """Take attribute `key` off the text between the gaps `start` and `end`; returns the op."""
        return self._rt_add(start, end, key, 0, REMOVE, expand)

    def sync_formats_from(self, other) -> int:
        """Take the format ops of `other` that this peer lacks; returns how many."""
        new = {op: f for op, f in other.formats.items() if op not in self.formats}
        self.formats.update(new)
        return len(new)

    def spans(self) -> tuple:
        """([(pos, len, {key: value})] in this adapter's unit, pending): what an editor paints,
        and the formats whose anchors this peer cannot place until its next text sync."""
        sp, pend = self._rt_peer().spans(
            [(f[0], f[1], f[2], f[3], op, f[4]) for op, f in sorted(self.formats.items())])
        unit = 2 if self.EDITS_USE_BYTE_OFFSETS else 0  # (pos, len, pos_bytes, len_bytes, attrs)
        return [(x[unit], x[unit + 1], x[4]) for x in sp], pend


class HipMerge(_Adapter):
    """Mirror of the reference's per-CRDT adapter for the GPU engine.

    `Upstream` (/root/reference/src/rope.rs:6-33): NAME, EDITS_USE_BYTE_OFFSETS, from_str,
    insert, remove, replace, len.  `Downstream` (:185-191): upstream_updates, apply_update.
    len() is where the merge happens (as Dt::len -> checkout_tip, rope.rs:133-136): it calls
    crdt_hip_merge on the shared device context.
    """

    NAME = "mi355x"
    _ctx: Context | None = None

    def __init__(self, log: OpLog):
        self.log = log

    def _rt_peer(self) -> OpLog:
        return self.log

    @classmethod
    def context(cls) -> Context:
        if cls._ctx is None:
            cls._ctx = Context(0)
        return cls._ctx

    @classmethod
    def from_str(cls, s: str) -> "HipMerge":
        log = OpLog()
        if s:
            log.insert(0, s)
        return cls(log)

    def clone(self) -> "HipMerge":
        return HipMerge(self.log.clone())

    def text(self) -> str:
        data, _ = self.context().merge(self.log)
        return data.decode("utf-8")

    def len(self) -> int:
        # the merge (Dt::len -> checkout_tip, rope.rs:133-136): codepoints of the merged text,
        # counted on the device (EDITS_USE_BYTE_OFFSETS = false)
        return self.context().merge_len(self.log)[0]

    # Downstream
    @classmethod
    def upstream_updates(cls, start_content: str, patches) -> tuple:
        up = cls.from_str(start_content)
        updates = []
        for pos, dele, ins in patches:
            v = up.log.version()
            up.replace(pos, pos + dele, ins)
            updates.append(up.log.encode_from(v))
        return cls.from_str(start_content), updates

    def apply_update(self, update: bytes) -> None:
        self.log.apply_update(update)


class HipDownstream(_Adapter):
    """`Downstream` (/root/reference/src/rope.rs:185-191) with the replica on the device.

    apply_update() queues the encoded update on the host; len() decodes every queued update on
    the device in one batch (crdt_hip_replica_apply_updates), merges the replica there and
    returns its visible codepoints; every other call decodes the queue first too.  clone() copies
    the replica device to device.  It is an `Upstream` (rope.rs:6-33) too: from_str, insert, remove
    and replace resolve the edit on the device (crdt_hip_replica_replace), so no host log is kept
    beside the replica.  This is the shape of the Rust adapter in INTEGRATION.md.
    """

    NAME = "mi355x-device"

    def __init__(self, replica: Replica):
        self.replica = replica
        self.pending: list = []

    def _rt_peer(self) -> Replica:
        self.flush()
        return self.replica

    @classmethod
    def upstream_updates(cls, start_content: str, patches) -> tuple:
        up, updates = HipMerge.upstream_updates(start_content, patches)
        ctx = HipMerge.context()
        return cls(Replica(ctx, up.log if up.log.view().n else None)), updates

    @classmethod
    def from_str(cls, s: str) -> "HipDownstream":
        d = cls(Replica(HipMerge.context()))
        if s:
            d.insert(0, s)
        return d

    def clone(self) -> "HipDownstream":
        c = HipDownstream(self.replica.clone())
        c.pending = list(self.pending)
        return c

    def apply_update(self, update: bytes) -> None:
        self.pending.append(update)

    def flush(self) -> None:
        if self.pending:
            self.replica.apply_updates(self.pending)
            self.pending = []

    def text(self) -> str:
        return self._rt_peer().merge()[0].decode("utf-8")

    def len(self) -> int:
        """The merged document's length in the adapter's unit (main.rs:68 asserts it): the merge's
        own count, cross-checked against the decoder's visible counter."""
        doc = self._rt_peer()
        unit = 1 if self.EDITS_USE_BYTE_OFFSETS else 0
        n, counter = doc.merge_len()[unit], doc.info()[1 + unit]
        if n != counter:
            raise CrdtHipError(-5, f"merged text has {n} {('codepoints', 'bytes')[unit]}, "
                                   f"the decoder counted {counter}")
        return n


class HipDownstreamBytes(HipDownstream):
    """HipDownstream for a caller that keeps its text as UTF-8 (EDITS_USE_BYTE_OFFSETS = true,
    rope.rs:8,16-19, as the cola and yrs adapters): insert, remove and replace take byte offsets,
    patches_since and sync_patches return byte patches, and len() is a byte length.  The offsets
    are translated on the device (crdt_hip.h, "byte offsets"); no text is kept on the host."""

    NAME = "mi355x-device-bytes"
    EDITS_USE_BYTE_OFFSETS = True

    def clone(self) -> "HipDownstreamBytes":
        c = HipDownstreamBytes(self.replica.clone())
        c.pending = list(self.pending)
        return c