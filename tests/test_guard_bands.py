"""The guard-band helper (tests/guard_bands.py) itself, on the CPU: the layouts and base alignment are the ones
asked for, `intact` sees a single changed element before the view, after it and in a pitch / plane gap (and
nothing else), and the poison lies where the GPU tests assume: one row or column past the view."""
import pytest
import torch

import guard_bands as gb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_embed_dense_alignment_and_padding(dtype):
    t = torch.randn(3, 5, 8).to(dtype)
    v, buf = gb.embed(t, fill=gb.POISON)
    assert buf.dim() == 1 and buf.dtype == dtype and v.dtype == dtype
    assert v.shape == t.shape and torch.equal(v, t) and v.is_contiguous()
    assert v.data_ptr() % 16 == 0 and v.data_ptr() % gb.ALIGN == 16
    item = t.element_size()
    first = (v.data_ptr() - buf.data_ptr()) // item
    last = first + t.numel() - 1
    assert first * item >= 65536 and (buf.numel() - 1 - last) * item >= 65536
    assert bool(torch.isnan(buf[:first]).all()) and bool(torch.isnan(buf[last + 1:]).all())
    assert gb.intact(v, buf, gb.POISON)


def test_embed_offsets_and_pads():
    t = torch.arange(12.0).reshape(3, 4)
    for off in (0, 16, 48, 256):
        v, buf = gb.embed(t, fill=1.0, pad_bytes=4096, offset_bytes=off)
        assert v.data_ptr() % gb.ALIGN == off
        assert v.data_ptr() - buf.data_ptr() >= 4096
        assert buf.data_ptr() + buf.numel() * 4 - (v.data_ptr() + 12 * 4) >= 4096


def test_embed_pitched_permuted_and_gapped():
    t = torch.randn(2, 5, 8)
    v, buf = gb.embed(t, fill=gb.SENTINEL, pitch=16, gap=64)
    assert v.stride() == (5 * 16 + 64, 16, 1) and torch.equal(v, t)
    base = (v.data_ptr() - buf.data_ptr()) // 4
    whole = buf[base:base + v.stride(0) * 2].reshape(2, -1)
    rows = whole[:, :5 * 16].reshape(2, 5, 16)
    assert bool((rows[:, :, 8:] == gb.SENTINEL).all())                  # every pitch gap holds the fill
    assert bool((whole[:, 5 * 16:] == gb.SENTINEL).all())               # and the gap between the planes
    assert gb.intact(v, buf, gb.SENTINEL)
    # the last two dims swapped in memory: a [z, rows, cols] operand stored cols-major with a pitch over rows
    v, buf = gb.embed(t, fill=gb.POISON, order=(0, 2, 1), pitch=5 + 8)
    assert v.stride() == (8 * 13, 1, 13) and torch.equal(v, t)
    assert v.transpose(1, 2).stride(2) == 1
    assert v.data_ptr() % gb.ALIGN == 16
    assert gb.intact(v, buf, gb.POISON)
    # batch innermost but one: a packed [B, N, 3, H, d]-like permutation
    p = torch.randn(2, 3, 4, 8)
    v, buf = gb.embed(p, fill=gb.POISON, order=(0, 2, 1, 3))
    assert v.stride() == (4 * 3 * 8, 8, 3 * 8, 1) and torch.equal(v, p)


@pytest.mark.parametrize("dtype,fill", [(torch.float32, gb.SENTINEL), (torch.bfloat16, gb.SENTINEL),
                                        (torch.float16, gb.SENTINEL), (torch.float32, gb.POISON),
                                        (torch.bfloat16, gb.POISON), (torch.int32, -1), (torch.uint8, 1)])
def test_intact_reports_single_changed_element(dtype, fill):
    t = torch.ones(2, 5, 8).to(dtype)
    v, buf = gb.embed(t, fill=fill, pitch=16, gap=32)
    assert float(torch.full((1,), fill, dtype=dtype).double()) == fill or fill != fill   # the fill is exact in dtype
    first = (v.data_ptr() - buf.data_ptr()) // t.element_size()
    last = first + v.stride(0) + 4 * 16 + 7
    spots = {"first of buf": 0, "just before": first - 1, "just after": last + 1, "last of buf": buf.numel() - 1,
             "pitch gap": first + 8, "end of pitch gap": first + 15, "last row's gap": first + 4 * 16 + 8,
             "plane gap": first + 5 * 16, "end of plane gap": first + v.stride(0) - 1}
    other = torch.zeros((), dtype=dtype)
    for where, i in spots.items():
        assert gb.intact(v, buf, fill), where
        keep = buf[i].clone()
        buf[i] = other
        assert not gb.intact(v, buf, fill), where
        assert gb.touched(v, buf, fill).tolist() == [i], where
        assert str(i - first) in gb.describe(v, buf, fill)
        buf[i] = keep
    # writing the view itself is not a guard violation, whatever the value
    v.fill_(other)
    v[1, 4, 7] = fill
    assert gb.intact(v, buf, fill)


def test_intact_nan_fill_is_bitwise_and_sees_other_nan():
    """A NaN fill compares by bit pattern: another NaN (sign flipped) written into the guard is a change."""
    v, buf = gb.embed(torch.zeros(4, 4), fill=gb.POISON)
    assert gb.intact(v, buf, gb.POISON)
    buf[3] = -buf[3]
    assert bool(torch.isnan(buf[3])) and not gb.intact(v, buf, gb.POISON)


def test_intact_over_several_views_of_one_buffer():
    """q, k, v of one packed buffer: the guard is what belongs to none of them."""
    packed, buf = gb.embed(torch.randn(2, 7, 3, 2, 8), fill=gb.POISON)
    q, k, v = packed.unbind(2)
    assert gb.intact([q, k, v], buf, gb.POISON)
    assert not gb.intact([q, k], buf, gb.POISON)                       # v's elements are not NaN
    with pytest.raises(AssertionError):
        gb.intact(torch.zeros(3), buf, gb.POISON)                      # not a view of buf


@pytest.mark.parametrize("order,pitch", [(None, None), (None, 24), ((1, 0), None), ((1, 0), 40)])
def test_poison_is_one_row_or_column_past_the_view(order, pitch):
    """What the GPU tests rely on: a product over the view extended by one row or one column (what a kernel
    with a missing tail mask would read) is NaN, in every layout, while the product over the view is not."""
    g = torch.Generator().manual_seed(0)
    M, K, N = 9, 16, 32
    A = torch.randn(M, K, generator=g)
    B = torch.randn(K, N, generator=g)
    a, abuf = gb.embed(A, fill=gb.POISON, order=order, pitch=pitch)
    assert not torch.isnan(a @ B).any()
    off = a.storage_offset()
    more_rows = abuf.as_strided((M + 1, K), a.stride(), off)
    more_cols = abuf.as_strided((M, K + 1), a.stride(), off)
    assert bool(torch.isnan(more_rows @ B)[M].any())
    assert bool(torch.isnan(more_cols @ torch.cat([B, torch.ones(1, N)])).any())
    one_before = abuf.as_strided((M, K), a.stride(), off - 1)
    assert bool(torch.isnan(one_before @ B).any())
    # 0 * poison is still NaN: a masked probability times a row past the end does not hide it
    assert bool(torch.isnan(torch.zeros(1, M + 1) @ more_rows).any())
