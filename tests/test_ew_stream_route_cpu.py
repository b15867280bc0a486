"""The library's own account of which element-wise passes take the streaming route (csrc/ew_stream.h), checked without a
GPU: pcaa_ew_route is a pure host function of (pass, dtype, rows, ch, alignment) and the switch.  Nothing is launched."""
import pytest

from opensetgaitrecognition_pcaa_amd import _lib

F32, BF16, SPLIT = 0, 1, 2                                     # PCAA_F32, PCAA_BF16, PCAA_SPLIT_F16
ACT_FWD, BWD_DY, BWD_DY_FUSED, MEANPOOL, IN_BWD, IN_APPLY = range(6)   # PCAA_EW_* of include/pcaa_hip.h
PORTED = (ACT_FWD, BWD_DY)
STREAM_CH = [8, 16, 64, 128, 256, 512, 1024, 2048]           # ch / 8 divides 256
RAGGED_CH = [4, 12, 20, 24, 96, 100, 1020, 1028, 4096]         # not a multiple of 8, or ch / 8 does not divide 256


@pytest.fixture()
def lib():
    lib = _lib.load()
    was = lib.pcaa_ew_stream_set(1)
    yield lib
    lib.pcaa_ew_stream_set(was)


def route(lib, *args):
    return lib.pcaa_ew_route(*args).decode()


def takes(kind, ch):
    """bn_act_fwd streams from 1024 channels on (narrower rows measured inside the classic route's spread)"""
    return ch >= 1024 if kind == ACT_FWD else True


@pytest.mark.parametrize("ch", STREAM_CH)
@pytest.mark.parametrize("kind", PORTED)
def test_bf16_and_supported_ch_stream(lib, kind, ch):
    for rows in (1, 7, 245760):
        assert route(lib, kind, BF16, rows, ch, 1) == ("stream" if takes(kind, ch) else "classic")


def test_the_flagship_shapes(lib):
    assert route(lib, ACT_FWD, BF16, 245760, 512, 1) == "classic"
    assert route(lib, ACT_FWD, BF16, 245760, 1024, 1) == "stream"
    assert route(lib, BWD_DY, BF16, 245760, 512, 1) == "stream"
    assert route(lib, BWD_DY, BF16, 245760, 1024, 1) == "stream"


@pytest.mark.parametrize("kind", PORTED)
def test_everything_else_is_classic(lib, kind):
    for ch in STREAM_CH:
        assert route(lib, kind, F32, 4096, ch, 1) == "classic"          # fp32 storage
        assert route(lib, kind, SPLIT, 4096, ch, 1) == "classic"        # the split images
        assert route(lib, kind, BF16, 4096, ch, 0) == "classic"         # a tensor that is not 16-byte aligned
        assert route(lib, kind, BF16, 0, ch, 1) == "classic"            # nothing to do: the launcher refuses it
    for ch in RAGGED_CH:
        assert route(lib, kind, BF16, 4096, ch, 1) == "classic"


def test_passes_that_were_not_ported_are_classic(lib):
    for kind in (BWD_DY_FUSED, MEANPOOL, IN_BWD, IN_APPLY, 99, -1):
        assert route(lib, kind, BF16, 245760, 512, 1) == "classic"
        assert lib.pcaa_ew_ring_depth(kind) == 0 and lib.pcaa_ew_wgs_per_cu(kind) == 0


def test_switch_off_is_classic_everywhere_and_reports_the_previous_setting(lib):
    assert lib.pcaa_ew_stream_set(0) == 1
    try:
        for kind in PORTED:
            for ch in STREAM_CH:
                assert route(lib, kind, BF16, 245760, ch, 1) == "classic"
        assert lib.pcaa_ew_stream_set(0) == 0
    finally:
        assert lib.pcaa_ew_stream_set(1) == 0
    assert route(lib, BWD_DY, BF16, 245760, 512, 1) == "stream"


def test_geometry_of_the_ported_passes(lib):
    for kind in PORTED:
        k, r = lib.pcaa_ew_wgs_per_cu(kind), lib.pcaa_ew_ring_depth(kind)
        # 16-32 KB in flight per CU: k workgroups x 256 lanes x 16 B x r rows x inputs
        inputs = 2 if kind == BWD_DY else 1
        assert 1 <= k <= 8 and 1 <= r <= 8
        assert 8 <= k * r * 4 * inputs <= 32


def test_abi_number_covers_the_new_entry_points(lib):
    assert lib.pcaa_abi_version() == _lib.ABI_VERSION >= 28
