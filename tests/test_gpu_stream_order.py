"""Cross-stream ordering through ppf_stream_arm / ppf_stream_wait_stream when the armed call enqueues something that is not a kernel
(a memset alone, a memset followed by a kernel) and after an armed call that failed in a replay.  Stream A is given about a millisecond
of device work (fills of a 1 GiB buffer, a few host microseconds each) in front of the operation under test, so a consumer on stream B that
did not wait for it reads the old values."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 4 * 1024 * 1024                   # 16 MiB of fp32
BUSY = 4                              # fills of the 1 GiB buffer queued on A in front of the operation under test (~0.25 ms each)


@pytest.fixture(scope="module")
def env():
    from protopformer_amd import _lib
    _lib.lib()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    x = torch.empty(N, dtype=torch.float32, device="cuda")
    y = torch.empty(N, dtype=torch.bfloat16, device="cuda")
    big = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    yield _lib, a, b, x, y, big
    del big


def _busy(big):
    for _ in range(BUSY):
        big.fill_(0.0)


def _fill_then_busy(a, x, big, value):
    with torch.cuda.stream(a):
        x.fill_(value)
        _busy(big)


def _cast_on_b_is_zero(_lib, a, b, x, y):
    _lib.call("ppf_stream_wait_stream", b.cuda_stream, a.cuda_stream)
    _lib.call("ppf_cast_f32_bf16", x, y, N, b.cuda_stream)
    torch.cuda.synchronize()
    return int(torch.count_nonzero(y.view(torch.int16))) == 0


def _case_a(_lib, a, b, x, y, big):
    y.fill_(3.0)
    torch.cuda.synchronize()
    _fill_then_busy(a, x, big, 1.0)
    _lib.call("ppf_stream_arm", a.cuda_stream, 1)
    _lib.call("ppf_memset_zero", x, N * 4, a.cuda_stream)             # an armed call without a kernel
    return _cast_on_b_is_zero(_lib, a, b, x, y)


def test_armed_memset_alone_is_waited_for(env):
    assert _case_a(*env)


def test_armed_memset_then_kernel_is_waited_for(env):
    _lib, a, b, x, _, big = env
    rows_dst, row_floats = 4096, N // 4096
    src = torch.ones(rows_dst // 2, row_floats, dtype=torch.float32, device="cuda")
    rows = torch.arange(1, rows_dst, 2, dtype=torch.int32, device="cuda")
    want = torch.zeros(rows_dst, row_floats, dtype=torch.float32, device="cuda")
    want[rows.long()] = 1.0
    torch.cuda.synchronize()
    _fill_then_busy(a, x, big, 7.0)
    _lib.call("ppf_stream_arm", a.cuda_stream, 1)
    _lib.call("ppf_scatter_rows", src, rows, x, rows_dst // 2, rows_dst, row_floats * 4, a.cuda_stream)     # memset, then a kernel
    _lib.call("ppf_stream_wait_stream", b.cuda_stream, a.cuda_stream)
    with torch.cuda.stream(b):
        got = x.view(rows_dst, row_floats).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_failed_armed_call_in_replay_leaves_the_stream_disarmed(env):
    _lib, a, b, x, y, big = env
    rec = _lib.Recorder()
    cast, wait = _lib._FAST["ppf_cast_f32_bf16"][0], _lib._FAST["ppf_stream_wait_stream"][0]
    # n = 7 fails the argument check of the cast (a multiple of 8 is required): rc != 0, nothing enqueued
    rec.cmds = [(_lib.Recorder.CALL, cast, (x.data_ptr(), y.data_ptr(), 7, a.cuda_stream), "ppf_cast_f32_bf16"),
                (_lib.Recorder.CALL, wait, (b.cuda_stream, a.cuda_stream), "ppf_stream_wait_stream")]
    assert _lib._arm_plan(rec.cmds) == {0: a.cuda_stream}
    with pytest.raises(RuntimeError, match="failed in replay"):
        _lib.replay(rec)
    # an eager launch on A, then work on A that is not the library's: a stream left armed would make B wait for the small kernel only
    y.fill_(3.0)
    torch.cuda.synchronize()
    x.fill_(1.0)
    torch.cuda.synchronize()
    _lib.call("ppf_cast_f32_bf16", x, y, 8, a.cuda_stream)
    with torch.cuda.stream(a):
        _busy(big)
        x.zero_()
    assert _cast_on_b_is_zero(_lib, a, b, x, y)
    assert _case_a(_lib, a, b, x, y, big)
