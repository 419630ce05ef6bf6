"""Row state without a GPU: the RowState container on CPU tensors, and what the header says about the four entries.

The container never interprets a record -- it regroups, moves and stores bytes -- so everything it does can be held to bits here, with NaN
payloads and -0.0 among them. The header checks pin the shape of the ABI (include/robustcap_hip.h): rc_save_rows / rc_load_rows take a
descriptor that carries the stream, rc_set_state takes none, so that tests/test_stream_cases_cpu.py, which lists every entry with a
`void* stream` parameter in the table of tests/test_gpu_stream_order.py, does not see them (their fenced cases are in
tests/test_gpu_row_state.py)."""
import io
import re
import struct

import pytest
import torch

from robustcap_amd import _lib
from robustcap_amd import config as cfg
from robustcap_amd.rowstate import HIDDEN, RowState

BYTES = 4 * (4 * sum(HIDDEN) + 512 + 160)              # (h, c) of two layers per net, x4l, x6l, the small block


def _records(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(0, 256, (n, BYTES), dtype=torch.uint8, generator=g)
    # a quiet NaN with a payload, a signalling one, -0.0 and a denormal in every record: bytes that float handling would change
    for k, word in enumerate((0x7FC00001, 0x7F800001, 0x80000000, 0x00000001)):
        d[:, 16 * k:16 * k + 4] = torch.tensor(list(struct.pack("<I", word)), dtype=torch.uint8)
    return d


def test_record_size_is_what_the_layout_adds_up_to():
    assert HIDDEN == (512, 512, 1280, 1024, 512, 512) == tuple(h for _, _, h, _ in cfg.NETS)
    assert 4 * sum(HIDDEN) == 17408 and BYTES == 72320 and BYTES % 16 == 0


def test_container_keeps_shape_and_refuses_what_is_not_records():
    s = RowState(_records(3), 1)
    assert len(s) == 3 and s.bytes_per_row == BYTES and s.format == 1 and s.hidden == HIDDEN and s.device.type == "cpu"
    assert "3 records" in repr(s)
    with pytest.raises(ValueError, match="uint8"):
        RowState(torch.zeros(3, BYTES), 1)
    with pytest.raises(ValueError, match="uint8"):
        RowState(torch.zeros(BYTES, dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="multiple of 16"):
        RowState(torch.zeros(2, 24, dtype=torch.uint8), 1)
    assert len(RowState(torch.zeros(0, BYTES, dtype=torch.uint8), 1)) == 0


def test_indexing_and_cat_regroup_records_exactly():
    d = _records(5, 1)
    s = RowState(d.clone(), 1)
    assert torch.equal(s[2].data, d[2:3]) and len(s[2]) == 1
    assert torch.equal(s[-1].data, d[4:5])
    assert torch.equal(s[[3, 0, 3]].data, d[[3, 0, 3]])
    assert torch.equal(s[torch.tensor([4, 1])].data, d[[4, 1]])
    assert torch.equal(s[1:4].data, d[1:4])
    with pytest.raises(IndexError):
        s[5]
    back = RowState.cat([s[[2, 0]], s[1], s[3:]])
    assert torch.equal(back.data, d[[2, 0, 1, 3, 4]]) and back.format == 1 and back.hidden == HIDDEN
    piece = s[0]
    piece.data[0, 100] ^= 255                                               # a copy: the source keeps its bits
    assert torch.equal(s.data, d)
    with pytest.raises(ValueError, match="nothing"):
        RowState.cat([])
    with pytest.raises(ValueError, match=r"format 2.*format 1"):
        RowState.cat([s, RowState(d.clone(), 2)])
    with pytest.raises(ValueError, match="hidden sizes"):
        RowState.cat([s, RowState(d.clone(), 1, (512,) * 6)])


def test_state_dict_round_trip_through_torch_save_keeps_every_bit():
    d = _records(4, 2)
    s = RowState(d.clone(), 1)
    sd = s.state_dict()
    assert set(sd) == {"data", "format", "hidden", "bytes_per_row"}
    assert isinstance(sd["format"], int) and isinstance(sd["bytes_per_row"], int) and all(isinstance(h, int) for h in sd["hidden"])
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    back = RowState.from_state_dict(torch.load(f, weights_only=True))
    assert torch.equal(back.data, d) and back.data.dtype == torch.uint8
    assert (back.format, back.hidden, back.bytes_per_row) == (1, HIDDEN, BYTES)
    assert torch.equal(back.cpu().data, d) and torch.equal(back.to("cpu").data, d)
    with pytest.raises(ValueError, match="missing"):
        RowState.from_state_dict({"data": d})
    with pytest.raises(ValueError, match="bytes per record"):
        RowState.from_state_dict(dict(sd, bytes_per_row=16))


def test_check_names_both_sides():
    s = RowState(_records(1), 1)
    s.check(1, HIDDEN, BYTES)
    with pytest.raises(ValueError, match=r"load_rows: the records have format 1,.*this context reads format 2,"):
        s.check(2, HIDDEN, BYTES)
    other = (512, 512, 1024, 1024, 512, 512)
    with pytest.raises(ValueError) as e:
        s.check(1, other, BYTES)
    assert str(HIDDEN) in str(e.value) and str(other) in str(e.value)
    with pytest.raises(ValueError, match=rf"{BYTES} bytes each.*{BYTES + 16} bytes each"):
        s.check(1, HIDDEN, BYTES + 16)


# ---------------------------------------------------------------------------------------------------------------- the header
def _header():
    with open(_lib.HEADER_PATH) as f:
        return f.read()


def test_header_declares_the_four_entries_and_the_descriptor():
    text = _header()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = " ".join(code.split())
    assert "int rc_row_state_bytes(rc_ctx* ctx, int64_t* bytes_per_row, int32_t* format);" in flat
    assert "int rc_save_rows(rc_ctx* ctx, const rc_row_io* io);" in flat
    assert "int rc_load_rows(rc_ctx* ctx, const rc_row_io* io);" in flat
    assert ("int rc_set_state(rc_ctx* ctx, const char* net, const float* h_host, const float* c_host, const uint8_t* row_mask_host);"
            in flat)
    m = re.search(r"typedef struct \{([^}]*)\} rc_row_io;", flat)
    assert m, "rc_row_io is not declared"
    fields = [" ".join(x.split()) for x in m.group(1).split(";") if x.strip()]
    assert fields == ["const int32_t* rows", "int32_t n", "void* blob", "int64_t bytes_per_row", "void* stream"], fields
    assert re.search(r"#define RC_ROW_STATE_FORMAT 1\b", text)
    # rc_set_state documents its synchronisation in the word rc_get_state uses for itself
    comment = text[:text.index("int rc_set_state(")].rsplit("/*", 1)[1]
    assert "Synchronises" in comment and "no stream" in comment
    # ... and the two stream-ordered entries say why their stream travels in the descriptor
    above = text[:text.index("} rc_row_io;")].rsplit("/* ----", 1)[1]
    assert "tests/test_stream_cases_cpu.py" in above and "DESCRIPTOR" in above and "tests/test_gpu_row_state.py" in above


def test_ctypes_descriptor_matches_the_header():
    import ctypes as C
    f = dict(_lib.RcRowIO._fields_)
    assert list(n for n, _ in _lib.RcRowIO._fields_) == ["rows", "n", "blob", "bytes_per_row", "stream"]
    assert f["n"] is C.c_int32 and f["bytes_per_row"] is C.c_int64 and f["rows"] is C.c_void_p and f["blob"] is C.c_void_p
    assert C.sizeof(_lib.RcRowIO) == 40                                     # 8 + 4 (+ 4) + 8 + 8 + 8: the C layout on LP64
    for name in ("rc_row_state_bytes", "rc_save_rows", "rc_load_rows", "rc_set_state"):
        assert name in _lib.SIGNATURES


def test_the_stream_case_table_does_not_see_them():
    """tests/test_stream_cases_cpu.py lists every entry whose parameter list names a stream; the row-state entries carry theirs in the
    descriptor (rc_set_state has none), so its own parser must not list them -- and must still see the entries it always saw."""
    import test_stream_cases_cpu as S
    entries = S._stream_entries()
    for name in ("rc_save_rows", "rc_load_rows", "rc_set_state", "rc_row_state_bytes"):
        assert name not in entries
        assert name in S._declarations(S._header())
    assert "rc_get_state" in entries and "rc_reset" in entries
