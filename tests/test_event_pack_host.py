"""Event preparation from the npz columns, host side (eemflow_amd/events.py, no GPU): the arithmetic that csrc/event_pack.hip
implements, restated in NumPy here, equals the host route bit for bit; the column reader, the staging layout and the route rule."""
import os
import re

import numpy as np
import pytest

from eemflow_amd import _lib, events as E, hrem
from eemflow_amd.voxelizer import EventSequence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = (0, 123456789, 1700000000000000123)                         # the last one is above 2^53: int64 -> double rounds
P_DTYPES = (np.int8, np.uint8, np.bool_, np.int64)


def columns(seed, n, base, p_dtype):
    """Sorted HREM-like columns with ties: t int64 [ns] from `base`, x and y uint16, p in {0, 1} as stored in the file."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, 50_000_000, n)).astype(np.int64) + base
    if n >= 8:
        t[n // 2:n // 2 + 3] = t[n // 2]                            # ties inside the set
        t[1] = t[0]                                                 # and at its start
    return t, rng.integers(0, 96, n).astype(np.uint16), rng.integers(0, 64, n).astype(np.uint16), rng.integers(0, 2, n).astype(p_dtype)


def todays_host_route(path):
    """hrem.get_compressed_events -> EventSequence(1e6, relative) -> astype('float'): what HREMEventFlow._read and the voxelizer's
    front-end do with an events npz today."""
    seq = EventSequence(None, {'height': 64, 'width': 96}, features=hrem.get_compressed_events(path), timestamp_multiplier=1e6,
                        convert_to_relative=True)
    return np.ascontiguousarray(seq.features.astype('float'))


def numpy_model(cols, scale_a=1e-9, scale_b=1e6, relative=True):
    """The kernel's arithmetic: every column as astype(float64); tt = (t * scale_a) * scale_b, two rounded products; tt - tt[0]."""
    t, x, y, p = (c.astype(np.float64) for c in cols)
    tt = (t * scale_a) * scale_b
    return np.stack([tt - tt[0] if relative else tt, x, y, p], axis=1)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("p_dtype", P_DTYPES)
def test_numpy_model_equals_the_host_route(tmp_path, base, p_dtype):
    t, x, y, p = columns(1, 5000, base, p_dtype)
    path = str(tmp_path / "events.npz")
    np.savez(path, t=t, x=x, y=y, p=p)
    want = todays_host_route(path)
    cols = E.read_event_columns(path)
    assert same_bits(numpy_model(cols), want)
    assert same_bits(E.host_events(cols), want)                     # the module's own host route is today's
    if base > 2 ** 53:
        assert np.any(t.astype(np.float64).astype(np.int64) != t)   # the conversion did round
    assert want[0, 0] == 0.0 and want[1, 0] == 0.0 and bool(np.all(np.diff(want[:, 0]) >= 0))


@pytest.mark.parametrize("p_dtype", P_DTYPES)
def test_read_event_columns_keeps_the_file_dtypes(tmp_path, p_dtype):
    t, x, y, p = columns(2, 257, 123456789, p_dtype)
    path = str(tmp_path / "events.npz")
    np.savez(path, t=t, x=x, y=y, p=p)
    ct, cx, cy, cp = E.read_event_columns(path)
    assert (ct.dtype, cx.dtype, cy.dtype) == (np.int64, np.uint16, np.uint16)
    assert np.array_equal(ct, t) and np.array_equal(cx, x) and np.array_equal(cy, y)
    want_p = 2 * p - 1                                              # in the column's own dtype: loader_utils.py:34
    assert cp.dtype == want_p.dtype and np.array_equal(cp, want_p)
    assert cp.dtype == {np.int8: np.int8, np.uint8: np.uint8, np.bool_: np.int64, np.int64: np.int64}[p_dtype]
    if p_dtype is np.uint8:
        assert set(np.unique(cp)) == {1, 255}                       # 0 -> 255, as in the reference
    else:
        assert set(np.unique(cp)) == {-1, 1}
    assert all(c.dtype in E.DTYPE_CODES for c in (ct, cx, cy, cp))


@pytest.mark.parametrize("n", [1, 7, 4001])
def test_staging_layout(n):
    sets = [columns(3, n, 0, np.int8), columns(4, n + 2, 0, np.bool_), columns(5, n, 0, np.int64)]
    sets[1] = sets[1][:3] + (sets[1][3].view(np.uint8),)
    offsets, total = E.staging_layout(sets)
    assert len(offsets) == 3 and all(len(o) == 4 for o in offsets)
    at = 0
    for cols, offs in zip(sets, offsets):                           # per set t | x | y | p, each start rounded up to 16 bytes
        for c, off in zip(cols, offs):
            assert off % 16 == 0 and off == (at + 15) // 16 * 16 and off - at < 16
            at = off + c.shape[0] * c.dtype.itemsize
    assert total == at
    m = n + 2
    assert offsets[0] == (0, (8 * n + 15) // 16 * 16, (8 * n + 15) // 16 * 16 + (2 * n + 15) // 16 * 16,
                          (8 * n + 15) // 16 * 16 + 2 * ((2 * n + 15) // 16 * 16))
    assert offsets[1][0] == (offsets[0][3] + n + 15) // 16 * 16 and offsets[1][3] + m <= offsets[2][0] < offsets[1][3] + m + 16
    # filling a buffer by that layout puts every column's bytes where the layout says
    host = np.full(total, 0xEE, np.uint8)
    E._fill_stage(host, sets, offsets)
    for cols, offs in zip(sets, offsets):
        for c, off in zip(cols, offs):
            assert np.array_equal(host[off:off + c.nbytes].view(c.dtype), c)


def test_route_rule():
    cols = columns(6, 500, 123456789, np.int8)
    cols = cols[:3] + (2 * cols[3] - 1,)
    assert E.route_of(cols) == 'device'
    swapped = cols[0].copy()
    swapped[[200, 300]] = swapped[[300, 200]]
    assert swapped[200] > swapped[201] and E.route_of((swapped,) + cols[1:]) == 'host'
    ft = cols[0].astype(np.float64)
    assert E.route_of((ft,) + cols[1:]) == 'device'
    ft[77] = np.nan
    assert E.route_of((ft,) + cols[1:]) == 'host'
    assert E.route_of((cols[0].astype(np.float32),) + cols[1:]) == 'host'       # NumPy forms t * 1e-9 in float32 there
    assert E.route_of((cols[0].astype(np.uint64),) + cols[1:]) == 'host'        # no code for it
    assert E.route_of((cols[0][:1],) + tuple(c[:1] for c in cols[1:])) == 'device'
    # the host route orders an unordered set exactly as today (argsort)
    got = E.host_events((swapped,) + cols[1:])
    feats = np.stack([swapped * 1e-9, cols[1], cols[2], cols[3]], axis=1).astype(np.float64)
    want = EventSequence(None, {'height': 64, 'width': 96}, features=feats, timestamp_multiplier=1e6, convert_to_relative=True).features
    assert same_bits(got, np.ascontiguousarray(want.astype('float')))


def test_an_empty_set_raises_what_the_host_route_raises(tmp_path):
    path = str(tmp_path / "events.npz")
    np.savez(path, t=np.zeros(0, np.int64), x=np.zeros(0, np.uint16), y=np.zeros(0, np.uint16), p=np.zeros(0, np.int8))
    with pytest.raises(ValueError) as today:
        todays_host_route(path)
    before = dict(E.route_counts)
    with pytest.raises(ValueError) as now:                          # raised on the host, before anything touches the GPU
        E.pack_events_many([E.read_event_columns(path)])
    assert str(now.value) == str(today.value)
    assert E.route_counts == before


def test_header_declares_the_entry_point_with_its_citation():
    header = open(os.path.join(REPO, "include", "eemflow_hip.h")).read()
    at = header.index("int eemflow_pack_events_many(")
    block = header[header.rindex("/*", 0, at):at]
    assert "Replaces:" in block and "loader_utils.py:26-37" in block and "loader_utils.py:352-397" in block
    assert int(re.search(r"#define EEMFLOW_PACK_MAX (\d+)", block).group(1)) == E.PACK_MAX == 32
    codes = {name: int(v) for name, v in re.findall(r"#define EEMFLOW_PACK_(U8|I8|U16|I16|I32|I64|F32|F64) (\d+)", block)}
    want = {"U8": np.uint8, "I8": np.int8, "U16": np.uint16, "I16": np.int16, "I32": np.int32, "I64": np.int64, "F32": np.float32,
            "F64": np.float64}
    assert {k: E.DTYPE_CODES[np.dtype(v)] for k, v in want.items()} == codes and E.DTYPE_CODES[np.dtype(np.bool_)] == codes["U8"]
    assert "eemflow_pack_events_many" in _lib.EXPORTS
    import eemflow_amd
    assert eemflow_amd.pack_events_many is E.pack_events_many and eemflow_amd.read_event_columns is E.read_event_columns
    from eemflow_amd.build import EXTRA, SOURCES
    assert "event_pack.hip" in SOURCES and "-ffp-contract=off" in EXTRA["event_pack.hip"]


def test_hrem_flag_is_off_by_default_and_the_cli_refuses_other_datasets():
    import inspect
    from eemflow_amd import cli
    assert inspect.signature(hrem.HREMEventFlow.__init__).parameters["device_events"].default is False
    for cmd in ("train", "test"):
        assert cli.build_parser().parse_args([cmd]).device_events is False
        assert cli.build_parser().parse_args([cmd, "--device_events"]).device_events is True
    on = cli.build_parser().parse_args(["train", "--device_events"])
    assert cli.device_events_kw(on, hrem.HREMEventFlow) == {"device_events": True}
    assert cli.device_events_kw(cli.build_parser().parse_args(["train"]), hrem.HREMEventFlow) == {}
    from eemflow_amd import mvsec
    with pytest.raises(SystemExit, match="--device_events"):
        cli.device_events_kw(on, mvsec.MvsecEventFlow)
