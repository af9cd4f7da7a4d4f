"""The four places where functional.py hands a row table to a kernel — _rows_f32, _rows_any, _dot_rows and the rows
spmm_csr gathers (_gather_rows) — decide per input: the same object back, or a copy.  The table below was written from the
four separate implementations that preceded the shared normaliser and pins every decision: identity where the tensor passes
through, dtype / contiguity / equal values where it is copied.  Host only: the decisions depend on dtype, strides and the
base address, none of which need a GPU."""
import pytest
import torch

from pangnn_amd import functional as PF

ROWS16 = (torch.bfloat16, torch.float16)
DTYPES = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


def _values(rows, cols, dtype):
    """small integers: exact in every one of the four formats, so a converted copy compares equal bit for bit"""
    return ((torch.arange(rows * cols, dtype=torch.float64) * 7) % 61 - 30).reshape(rows, cols).to(dtype)


def _flat_off(dtype, elements, cols=64):
    """a contiguous [5, cols] whose base lies `elements` elements into a (64-byte aligned) buffer"""
    buf = torch.zeros(5 * cols + elements, dtype=dtype)
    t = buf[elements:].view(5, cols)
    t.copy_(_values(5, cols, dtype))
    return t


CASES = {
    "contiguous": lambda dt: _values(5, 64, dt),
    "column_window": lambda dt: _values(5, 128, dt)[:, 64:128],
    "odd_row_stride": lambda dt: _values(5, 66, dt)[:, :64],                 # row stride 66
    "base_off_one_element": lambda dt: _values(5, 65, dt)[:, 1:],            # float32: 4 bytes off; row stride 65
    "transposed": lambda dt: _values(64, 5, dt).t(),
    "row_stride_68": lambda dt: _values(5, 68, dt)[:, :64],                  # a multiple of 4 elements, not of 8
    "contiguous_base_off_one_element": lambda dt: _flat_off(dt, 1),          # contiguous, only the base address is off
    "contiguous_base_off_8_bytes": lambda dt: _flat_off(dt, 8 // torch.empty(0, dtype=dt).element_size()),
    "expanded_row": lambda dt: _values(1, 64, dt).expand(5, 64),             # row stride 0: the rows overlap
    "width_48": lambda dt: _values(5, 48, dt),                               # 2-byte rows of this width are not gathered as stored
}

# case -> site -> (float32 input, bfloat16 / float16 input): "same" = the object itself, "f32" = a contiguous float32 copy,
# "16" = a contiguous copy in the stored 2-byte type.  float64 input is always a contiguous float32 copy.
S, F, H = "same", "f32", "16"
TABLE = {
    #                                   _rows_f32   _rows_any   _dot_rows   _gather_rows
    "contiguous":                       ((S, F),    (S, S),     (S, S),     (S, S)),
    "column_window":                    ((S, F),    (S, S),     (S, S),     (F, S)),
    "odd_row_stride":                   ((F, F),    (F, H),     (F, H),     (F, H)),
    "base_off_one_element":             ((F, F),    (F, H),     (F, H),     (F, H)),
    "transposed":                       ((F, F),    (F, H),     (F, H),     (F, H)),
    "row_stride_68":                    ((S, F),    (S, H),     (S, S),     (F, S)),
    "contiguous_base_off_one_element":  ((S, F),    (S, S),     (F, H),     (S, S)),
    "contiguous_base_off_8_bytes":      ((S, F),    (S, S),     (F, S),     (S, S)),
    "expanded_row":                     ((F, F),    (F, H),     (F, H),     (F, S)),
    "width_48":                         ((S, F),    (S, S),     (S, F),     (S, F)),
}
SITES = ("_rows_f32", "_rows_any", "_dot_rows", "_gather_rows")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("site", SITES)
def test_row_normaliser_decision(site, case, dtype):
    t = CASES[case](dtype)
    before = t.clone()
    out = getattr(PF, site)(t)
    want = F if dtype == torch.float64 else TABLE[case][SITES.index(site)][1 if dtype in ROWS16 else 0]
    if want == S:
        assert out is t
    else:
        assert out is not t and out.data_ptr() != t.data_ptr()
        assert out.dtype == (torch.float32 if want == F else dtype)
        assert out.is_contiguous() and out.data_ptr() % 16 == 0
        assert out.shape == t.shape
        assert torch.equal(out.double(), t.double())
    assert torch.equal(t, before)                # the input is never written


def test_the_two_width_sets_are_stated_once():
    assert PF.GATHER_WIDTHS == (32, 64, 128, 256)
    assert PF.PART_SUM_WIDTHS == (16, 32, 64, 128, 256)
