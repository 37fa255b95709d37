"""Stream slots on the host side (include/nam_hip.h: nam_hip_batch_restart_streams, nam_hip_batch_stream_state_size,
nam_hip_batch_get_stream_state, nam_hip_batch_set_stream_state): a NULL batch is refused before any device call, and the Python
wrappers are there. What the calls do on a device: tests/test_gpu_stream_state.py; the blob format: tests/test_stream_state_format.py."""
import ctypes
import inspect

STREAM_STATE_SYMBOLS = ["nam_hip_batch_restart_streams", "nam_hip_batch_stream_state_size", "nam_hip_batch_get_stream_state",
                        "nam_hip_batch_set_stream_state"]


def test_null_batch_is_an_invalid_argument(nam_lib):
    nam = nam_lib
    L = nam.load_library()
    ids = (ctypes.c_int * 2)(0, 1)
    buf = ctypes.create_string_buffer(256)
    size = ctypes.c_int64(-7)
    assert L.nam_hip_batch_restart_streams(None, ids, 2, 1) == nam.ERR_INVALID_ARGUMENT
    assert b"nam_hip_batch_restart_streams" in L.nam_hip_last_error()
    assert L.nam_hip_batch_restart_streams(None, None, 0, 0) == nam.ERR_INVALID_ARGUMENT
    assert L.nam_hip_batch_stream_state_size(None, 0) == nam.ERR_INVALID_ARGUMENT
    assert b"nam_hip_batch_stream_state_size" in L.nam_hip_last_error()
    assert L.nam_hip_batch_get_stream_state(None, 0, buf, 256, ctypes.byref(size)) == nam.ERR_INVALID_ARGUMENT
    assert b"nam_hip_batch_get_stream_state" in L.nam_hip_last_error()
    assert size.value == 0  # (no size to report)
    assert L.nam_hip_batch_get_stream_state(None, 0, buf, 256, None) == nam.ERR_INVALID_ARGUMENT
    assert L.nam_hip_batch_set_stream_state(None, 0, buf.raw, 256) == nam.ERR_INVALID_ARGUMENT
    assert b"nam_hip_batch_set_stream_state" in L.nam_hip_last_error()


def test_the_symbols_are_part_of_the_abi_list(nam_lib):
    for name in STREAM_STATE_SYMBOLS:
        assert name in nam_lib.ABI_SYMBOLS
        assert hasattr(nam_lib.load_library(), name)
    assert len(nam_lib.ABI_SYMBOLS) == len(set(nam_lib.ABI_SYMBOLS)) == 45


def test_python_wrappers_exist(nam_lib):
    B = nam_lib.Batch
    assert list(inspect.signature(B.restart_streams).parameters) == ["self", "stream_ids", "prewarm"]
    assert inspect.signature(B.restart_streams).parameters["stream_ids"].default is None
    assert inspect.signature(B.restart_streams).parameters["prewarm"].default is True
    assert list(inspect.signature(B.get_stream_state).parameters) == ["self", "stream"]
    assert list(inspect.signature(B.set_stream_state).parameters) == ["self", "stream", "blob"]


def test_version_prefix_is_unchanged(nam_lib):
    assert nam_lib.load_library().nam_hip_version().decode().startswith("nam_hip 0.2.6")
