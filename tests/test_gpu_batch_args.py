"""Argument checks of every public device wrapper in batch.py: the TYPE of the exception for a
CPU tensor, a wrong dtype, a non-contiguous tensor, a per-packet tensor of n - 1 / n + 1 entries,
descriptor arrays of different sizes, an empty ``first``, align_log2 outside the wrapper's range,
and (with two GPUs) a descriptor or an output on the other device.  Every case raises before
any launch: a pointer of the wrong size or device must never reach a kernel."""
import pytest
import torch

from rustnetworkstack_amd import _lib
from rustnetworkstack_amd import batch as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 130  # two full 64-packet batches and a partial one
L4, L6 = bytes([10, 0, 0, 1]), bytes(range(16))


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def z(n, dtype, device=DEV):
    return torch.zeros(n, dtype=dtype, device=device)


class Case:
    """One wrapper: ``call(**tensors)`` with valid arguments built by ``make(device)``.
    ``per_packet``: its optional tensors of exactly n entries (name -> dtype), ``pairs``:
    descriptor arrays that must agree in size, ``align``: its align_log2 range."""

    def __init__(self, name, call, make, per_packet, pairs=(), align=None, align_error=ValueError):
        self.name, self.call, self.make, self.per_packet, self.pairs = name, call, make, per_packet, pairs
        self.align, self.align_error = align, align_error

    def __repr__(self):
        return self.name


def explicit(device=DEV):
    return dict(arena=z(4096, torch.uint8, device), off=z(N, torch.int64, device), length=z(N, torch.int32, device))


def packed(device=DEV):
    return dict(arena=z(4096, torch.uint8, device), blk_off=z(3, torch.int64, device),
                len16=z(N, torch.int16, device))


def chain(device=DEV):
    return dict(arena=z(4096, torch.uint8, device), frag_off=z(2 * N, torch.int64, device),
                frag_len=z(2 * N, torch.int32, device), first=z(N + 1, torch.int32, device))


def strided_rx(device=DEV):
    return dict(arena=z(N * 64, torch.uint8, device), len16=z(N, torch.int16, device))


def strided(device=DEV):
    return dict(arena=z(N * 64, torch.uint8, device))


def compact_chain(device=DEV):
    return dict(arena=z(4096, torch.uint8, device), head_blk_off=z(3, torch.int64, device),
                head_len8=z(N, torch.uint8, device), pay_blk_off=z(3, torch.int64, device),
                pay_len16=z(N, torch.int16, device))


U16, U8 = torch.uint16, torch.uint8
EXPL = (("off", "length"),)
FRAG = (("frag_off", "frag_len"),)
CASES = [
    Case("csum_batch", lambda arena, off, length, **k: B.csum_batch(arena, off, length, **k), explicit,
         dict(seed=U16, out=U16), EXPL),
    Case("PreparedBatch", lambda arena, off, length, **k: B.PreparedBatch(arena, off, length, **k), explicit,
         dict(seed=U16, out=U16), EXPL),
    Case("csum_batch_packed", lambda arena, blk_off, len16, **k: B.csum_batch_packed(arena, blk_off, len16, **k),
         packed, dict(seed=U16, out=U16), align=(0, 12)),
    Case("PackedBatch", lambda arena, blk_off, len16, **k: B.PackedBatch(arena, blk_off, len16, **k), packed,
         dict(seed=U16, out=U16), align=(0, 12)),
    Case("csum_batch_strided", lambda arena, **k: B.csum_batch_strided(arena, N, 64, 40, **k), strided,
         dict(seed=U16, out=U16)),
    Case("StridedBatch", lambda arena, **k: B.StridedBatch(arena, N, 64, 40, **k), strided, dict(seed=U16, out=U16)),
    Case("csum_chain", lambda arena, frag_off, frag_len, first, **k: B.csum_chain(arena, frag_off, frag_len, first, **k),
         chain, dict(seed=U16, out=U16), FRAG),
    Case("csum_chain_fill",
         lambda arena, frag_off, frag_len, first, **k: B.csum_chain_fill(arena, frag_off, frag_len, first, **k),
         chain, dict(seed=U16, field=U16, out=U16), FRAG),
    Case("csum_fill", lambda arena, off, length, **k: B.csum_fill(arena, off, length, **k), explicit,
         dict(seed=U16, field=U16, out=U16), EXPL),
    Case("csum_fill_packed", lambda arena, blk_off, len16, **k: B.csum_fill_packed(arena, blk_off, len16, **k), packed,
         dict(seed=U16, field=U16, out=U16), align=(4, 12)),
    Case("rx_verify", lambda arena, off, length, **k: B.rx_verify(arena, off, length, L4, L6, **k), explicit,
         dict(status=U8, l4_sum=U16), EXPL),
    Case("rx_verify_chain",
         lambda arena, frag_off, frag_len, first, **k: B.rx_verify_chain(arena, frag_off, frag_len, first, L4, L6, **k),
         chain, dict(status=U8, l4_sum=U16), FRAG),
    # rx_verify_packed leaves align_log2 to the C ABI, which answers RNS_E_INVALID before any launch
    Case("rx_verify_packed", lambda arena, blk_off, len16, **k: B.rx_verify_packed(arena, blk_off, len16, L4, L6, **k),
         packed, dict(status=U8, l4_sum=U16), align=(4, 12), align_error=_lib.ChecksumError),
    Case("rx_verify_strided", lambda arena, len16, **k: B.rx_verify_strided(arena, 64, len16, L4, L6, **k), strided_rx,
         dict(status=U8, l4_sum=U16)),
    Case("tx_fill", lambda arena, off, length, **k: B.tx_fill(arena, off, length, **k), explicit, dict(status=U8), EXPL),
    Case("tx_fill_packed", lambda arena, blk_off, len16, **k: B.tx_fill_packed(arena, blk_off, len16, **k), packed,
         dict(status=U8), align=(4, 12)),
    Case("tx_fill_chain",
         lambda arena, frag_off, frag_len, first, **k: B.tx_fill_chain(arena, frag_off, frag_len, first, **k), chain,
         dict(status=U8), FRAG),
    Case("tx_fill_chain_packed", lambda arena, head_blk_off, head_len8, pay_blk_off, pay_len16, **k:
         B.tx_fill_chain_packed(arena, head_blk_off, head_len8, pay_blk_off, pay_len16, **k), compact_chain,
         dict(status=U8), (("head_len8", "pay_len16"),)),
]
by_name = pytest.mark.parametrize("case", CASES, ids=repr)


def test_every_device_wrapper_is_covered():
    """The table names every public callable of batch.py that takes an arena and descriptor
    tensors (the layout helpers, the socket I/O, the host-resident batchers, the buffer fill and
    the multi-device launcher take none, or a shard list)."""
    host_side = {"packed_layout", "tx_chain_packed_layout", "recv_batch", "recv_batch_packed", "recv_batch_chain",
                 "send_batch", "send_batch_chain", "PinnedBuffer", "HostBatcher", "MultiHostBatcher",
                 "csum_batch_multi_dev", "fill_splitmix64"}
    public = {k for k, v in vars(B).items() if callable(v) and not k.startswith("_")
              and getattr(v, "__module__", None) == B.__name__}
    assert public - host_side == {c.name for c in CASES}


@by_name
def test_cpu_tensor(case):
    args = case.make()
    for name in args:
        with pytest.raises(ValueError, match="no CPU fallback"):
            case.call(**{**args, name: args[name].cpu()})
    for name, dt in case.per_packet.items():
        with pytest.raises(ValueError, match="no CPU fallback"):
            case.call(**args, **{name: z(N, dt, "cpu")})


@by_name
def test_wrong_dtype(case):
    args = case.make()
    for name, t in args.items():
        with pytest.raises(TypeError):
            case.call(**{**args, name: z(t.numel(), torch.float32)})
    for name in case.per_packet:
        with pytest.raises(TypeError):
            case.call(**args, **{name: z(N, torch.int32)})


@by_name
def test_non_contiguous(case):
    args = case.make()
    for name, t in args.items():
        with pytest.raises(ValueError):
            case.call(**{**args, name: z(2 * t.numel(), t.dtype)[::2]})
    for name, dt in case.per_packet.items():
        with pytest.raises(ValueError):
            case.call(**args, **{name: z(2 * N, dt)[::2]})


@by_name
@pytest.mark.parametrize("delta", [-1, 1])
def test_per_packet_tensor_of_the_wrong_size(case, delta):
    args = case.make()
    for name, dt in case.per_packet.items():
        with pytest.raises(ValueError):
            case.call(**args, **{name: z(N + delta, dt)})


@by_name
def test_descriptor_sizes_differ(case):
    args = case.make()
    for a, b in case.pairs:
        for name in (a, b):
            with pytest.raises(ValueError):
                case.call(**{**args, name: args[name][:-1]})
    if "first" in args:
        with pytest.raises(ValueError):
            case.call(**{**args, "first": args["first"][:0]})
    if "blk_off" in args:  # fewer than one offset per 64 packets
        with pytest.raises(ValueError):
            case.call(**{**args, "blk_off": args["blk_off"][:2]})


@by_name
def test_align_log2_out_of_range(case):
    args = case.make()
    if case.name == "tx_fill_chain_packed":
        lo, hi, kw, err = 4, 12, "pay_align_log2", ValueError
    elif case.align is None:
        return
    else:
        (lo, hi), kw, err = case.align, "align_log2", case.align_error
    for bad in ([lo - 1] if lo else []) + [hi + 1]:
        with pytest.raises(err):
            case.call(**args, **{kw: bad})


@by_name
def test_tensor_on_another_device(case):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    args = case.make()
    for name in args:
        if name != "arena":
            with pytest.raises(ValueError):
                case.call(**{**args, name: args[name].to("cuda:1")})
    for name, dt in case.per_packet.items():
        with pytest.raises(ValueError):
            case.call(**args, **{name: z(N, dt, "cuda:1")})
