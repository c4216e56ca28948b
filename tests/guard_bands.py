"""Guard bands around kernel operands: views embedded in a larger, filled buffer, so a test can tell a
stray write (the fill around an output changed) and a stray read that reaches a stored value (NaN poison
around an input turns up in the result) from a correct kernel, and exercises bases, pitches and plane
strides that are not those of a freshly allocated dense tensor.

    view, buf = embed(t, fill=POISON)            # an input: NaN all around (and in every pitch gap)
    out, obuf = embed(torch.full(shape, POISON), fill=SENTINEL, pitch=N + 8)
    kernel(view, out)
    assert not torch.isnan(out).any()            # every element written, nothing read from the poison
    assert intact(out, obuf, SENTINEL)           # nothing written beside the view
    assert intact(view, buf, POISON)             # inputs not written

A plain module (like op_cases.py): no fixtures, nothing GPU-specific; tensors live where `t` lives."""
import torch

POISON = float("nan")       # around inputs: any read that reaches a stored value shows as NaN
SENTINEL = -24576.0         # around outputs: finite, exact in bf16 / fp16 / fp32 (-1.5 * 2^14), far off any result
ALIGN = 512                 # the caching allocator's granularity: a fresh tensor's base is a multiple of it

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def embed(t, *, fill, pad_bytes=65536, offset_bytes=16, pitch=None, order=None, gap=0):
    """(view, buf): `buf` is one flat buffer of t.dtype filled with `fill`; `view` is a view into it with t's
    shape and values whose first element sits at least `pad_bytes` into buf, `offset_bytes` past a 512-B
    boundary (16: aligned for 16-B loads, and not like a freshly allocated tensor), followed by at least
    `pad_bytes` more of fill.

    Memory layout: t's dims in `order` (outermost first; default as they are, i.e. dense like a contiguous t),
    the innermost with stride 1, the next with stride `pitch` elements (default: the innermost extent; larger
    leaves fill between rows), the ones outside dense over that, the third-innermost with `gap` more elements
    of fill between its planes. order=(0, 2, 1) stores a [z, rows, cols] operand cols-major, etc."""
    nd = t.dim()
    order = tuple(range(nd)) if order is None else tuple(order)
    assert sorted(order) == list(range(nd)) and nd >= 1
    item = t.element_size()
    assert pad_bytes % item == 0 and offset_bytes % item == 0 and 0 <= offset_bytes < ALIGN
    ext = [t.shape[d] for d in order]                     # extents in memory order
    inner = ext[-1]
    pitch = inner if pitch is None else int(pitch)
    assert pitch >= inner and gap >= 0 and (pitch == inner or nd >= 2) and (gap == 0 or nd >= 3)
    mstr = [0] * nd                                       # strides in memory order
    mstr[-1] = 1
    if nd >= 2:
        mstr[-2] = pitch
    for i in range(nd - 3, -1, -1):
        mstr[i] = mstr[i + 1] * ext[i + 1] + (gap if i == nd - 3 else 0)
    span = 1 + sum((e - 1) * s for e, s in zip(ext, mstr)) if t.numel() else 0
    pad = pad_bytes // item
    buf = torch.full((2 * pad + (ALIGN + offset_bytes) // item + span,), fill, dtype=t.dtype, device=t.device)
    base = buf.data_ptr() + pad_bytes
    start = (-(-base // ALIGN) * ALIGN + offset_bytes - buf.data_ptr()) // item
    strides = [0] * nd
    for i, d in enumerate(order):
        strides[d] = mstr[i]
    view = buf.as_strided(tuple(t.shape), tuple(strides), start)
    view.copy_(t)
    return view, buf


def _outside(views, buf):
    """bool mask over buf: True where an element belongs to none of `views` (views into buf)."""
    if isinstance(views, torch.Tensor):
        views = [views]
    item = buf.element_size()
    m = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for v in views:
        assert v.dtype == buf.dtype and v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr(), \
            "not a view of this buffer"
        off = (v.data_ptr() - buf.data_ptr()) // item
        m.as_strided(tuple(v.shape), tuple(v.stride()), off).fill_(False)
    return m


def touched(views, buf, fill):
    """Flat indices into buf (ascending) of the elements outside `views` (one view or a list of views into buf)
    that no longer hold `fill`. The comparison is by bit pattern against torch.full(..., fill, dtype=buf.dtype):
    exact for a bf16 / fp16 sentinel and for a NaN fill (a kernel that does not write keeps the very bits)."""
    bits = _BITS[buf.element_size()]
    want = torch.full((1,), fill, dtype=buf.dtype, device=buf.device).view(bits)
    bad = (buf.view(bits) != want) & _outside(views, buf)
    return bad.nonzero().flatten()


def intact(views, buf, fill):
    """True only if every element of buf that is not an element of `views` still holds `fill`."""
    return touched(views, buf, fill).numel() == 0


def describe(views, buf, fill, limit=6):
    """For assertion messages: where the first touched elements lie relative to the (first) view's base."""
    idx = touched(views, buf, fill)
    v = views if isinstance(views, torch.Tensor) else views[0]
    base = (v.data_ptr() - buf.data_ptr()) // buf.element_size()
    rel = [int(i) - base for i in idx[:limit]]
    return f"{idx.numel()} guard element(s) changed; offsets from the view's base (elements): {rel}, " \
           f"view shape {tuple(v.shape)} strides {tuple(v.stride())}"
