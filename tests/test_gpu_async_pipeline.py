"""The asynchronous decode pipeline: jxlhip_decode_batch(..., synchronize=0) + jxlhip_finish, three workspace slots, three streams.

The batches are the table of tests/async_util.py (tests/test_async_cases.py holds its preconditions).  The reference of every output
is the same file decoded with synchronize=True by a fresh decoder under the same options, and equality is byte for byte: the
asynchronous route may change when a stage runs, never a bit.  The synchronous references themselves are pinned once, in the `jobs`
fixture: lossless files against their source pixels, lossy ones the oracle reads against the oracle under
test_gpu_parity.check_pixels; every test pins one lossy output of its own that way as well.

Nothing overlaps by itself at these sizes (a batch is finished before the next one is parsed), so the tests that need batches in
flight hold the caller's stream back with a delay kernel: the LF and HF chains of the next batches then complete on the decoder's own
streams while every pixel stage waits."""
import time

import numpy as np
import pytest

import async_util as AU
import downscale_util as DU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from test_gpu_parity import check_pixels

pytestmark = pytest.mark.gpu

FILL = 0xAA
OK, DECODE_ERROR = api.DECODER_STATUS.index("Ok"), api.DECODER_STATUS.index("DecodeError")
MAX_DELAY_MS = 400.0      # requested with a margin of a tenth; held_for() asserts that no delay lasted longer than 500 ms
HOLD_MS = 200.0           # the delay of the tests that only need a stream held while the host submits a few batches


class Job:
    """One decode_batch call: files, the bytes each output holds, the expected bytes (None: a file that fails), options."""

    def __init__(self, files, sizes, want, options=None, cases=None):
        self.files, self.sizes, self.want, self.options, self.cases = files, sizes, want, options or {}, cases

    def outputs(self):
        import torch
        return [torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for n in self.sizes]


def _nbytes(case, options):
    h, w, c = AU.out_shape(case, options)
    return h * w * c * np.dtype(case.dtype).itemsize


def submit(dec, job, outs, stream=None, synchronize=False, raise_on_error=True):
    """Options are read at submit time: the job's are set for this call only."""
    opts = dict(AU.DEFAULTS, **job.options)
    for k, v in opts.items():
        assert dec.set_option(k, v) == 1, k
    try:
        return dec.decode_batch(job.files, [o.data_ptr() for o in outs], None, stream.cuda_stream if stream is not None else None,
                                synchronize, raise_on_error)
    finally:
        for k, v in AU.DEFAULTS.items():
            dec.set_option(k, v)


def compare(job, outs, what=""):
    for k, (o, want) in enumerate(zip(outs, job.want)):
        if want is None:
            continue
        got = o.cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want), "%s file %d: %d of %d bytes differ from the synchronous decode" % (what, k, int((got != want).sum()), got.size)


@pytest.fixture(scope="module")
def table(oracle):
    return AU.table(oracle)


@pytest.fixture(scope="module")
def oracle_pixels(oracle):
    memo = {}

    def of(case):
        if id(case) not in memo:
            memo[id(case)] = oracle.decode(case.data).pixels
        return memo[id(case)]
    return of


@pytest.fixture(scope="module")
def jobs(table, oracle_pixels):
    """The table as jobs whose expected bytes come from a fresh decoder per batch, synchronize=True, same options; computed once and
    left alone.  The references are pinned here: lossless against the source, oracle-readable lossy files against the oracle."""
    import torch
    out = []
    for b in table:
        job = Job(b.files, [_nbytes(c, b.options) for c in b.cases], None, b.options, b.cases)
        dec = api.Decoder(0)
        try:
            outs = job.outputs()
            torch.cuda.synchronize()
            assert submit(dec, job, outs, synchronize=True) == [OK] * len(b.cases)
            job.want = [o.cpu().numpy() for o in outs]
        finally:
            dec.close()
        for c, want in zip(b.cases, job.want):
            px = want.view(c.dtype).reshape(AU.out_shape(c, b.options))
            if c.source is not None:
                ref = DU.box_mean_int(c.source) if b.options.get("downscale") == 8 else c.source
                assert np.array_equal(px, ref), (b.index, c.kind)
            elif c.oracle_ref and not b.options.get("downscale"):
                check_pixels(px, oracle_pixels(c))
        out.append(job)
    return out


@pytest.fixture
def dec():
    """A decoder of the test's own: the session decoder's slot state is shared with every other module."""
    d = api.Decoder(0)
    yield d
    d.close()


def pin_one_lossy(jobs_run, outs_run, oracle_pixels):
    """One lossy output of the run against the oracle (check_pixels): the asynchronous result, not only its reference."""
    for job, outs in zip(jobs_run, outs_run):
        if job.cases is None or job.options.get("downscale"):
            continue
        for c, o, want in zip(job.cases, outs, job.want):
            if c is not None and c.oracle_ref and want is not None:
                check_pixels(o.cpu().numpy().view(c.dtype).reshape(c.shape), oracle_pixels(c))
                return
    raise AssertionError("the run holds no lossy file the oracle reads")


# ---------------------------------------------------------------- the delay that holds a stream back
def _timed_sleep(stream, cycles):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record()
        torch.cuda._sleep(int(cycles))
        b.record()
    return a, b


def cycles_per_ms(stream):
    """Of torch.cuda._sleep's counter, measured on the stream in front of every delay (the clock it counts may have changed since the
    last one): a short spin to warm up, then spins of about 5 ms until one lasted 4 ms."""
    cycles, rate = 100000, None
    for _ in range(4):
        a, b = _timed_sleep(stream, cycles)
        stream.synchronize()
        ms = max(a.elapsed_time(b), 1e-3)
        rate = cycles / ms
        if ms >= 4.0:
            break
        cycles = int(rate * 5.0)
    return rate


def hold(stream, ms):
    """Enqueues a delay of at least `ms` on the stream; returns its (start, end) events for held_for()."""
    assert ms <= MAX_DELAY_MS
    return _timed_sleep(stream, cycles_per_ms(stream) * ms * 1.1)


def held_for(events, ms):
    """The delay lasted at least `ms` and no longer than the half second a test may wait: a condition of the test, not a figure."""
    lasted = events[0].elapsed_time(events[1])
    assert ms <= lasted <= 500.0, (ms, lasted)
    return lasted


# ---------------------------------------------------------------- 1. seven batches in flight, one finish()
def test_seven_batches_one_finish(dec, jobs, oracle_pixels):
    import torch
    for order in (jobs, jobs[::-1]):      # the second round on the same decoder: every slot shrinks or grows against what it held
        dec.stage_totals(reset=True)
        outs = [j.outputs() for j in order]
        torch.cuda.synchronize()
        for j, o in zip(order, outs):
            assert submit(dec, j, o) == [OK] * len(j.files)
        dec.finish()
        assert dec.stage_totals()[1] == len(order) == 7
        for k, (j, o) in enumerate(zip(order, outs)):
            compare(j, o, "batch %d" % k)
        pin_one_lossy(order, outs, oracle_pixels)


# ---------------------------------------------------------------- 2. forced out-of-order execution
def _sync_decode_ms(run):
    """Wall time of the synchronous decode of the jobs on a warm decoder of their own."""
    import torch
    d = api.Decoder(0)
    try:
        outs = [j.outputs() for j in run]
        torch.cuda.synchronize()
        for timed in (False, True):
            t0 = time.perf_counter()
            for j, o in zip(run, outs):
                submit(d, j, o, synchronize=True)
            ms = (time.perf_counter() - t0) * 1e3
        return ms
    finally:
        d.close()


def test_entropy_chains_run_ahead_of_a_held_pixel_stream(dec, jobs, oracle_pixels):
    """Three batches behind a delay on the caller's stream: their LF and HF chains run at once on the decoder's streams, every pixel
    stage (early noise, alpha reduce, Modular, compose, orient included) waits.  The fourth batch wants slot 0 back: the host blocks
    until batch 0 is through."""
    import torch
    run = jobs[:4]
    target = min(MAX_DELAY_MS, max(100.0, 5.0 * _sync_decode_ms(run[:3])))
    outs = [j.outputs() for j in run]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a, b = hold(s, target)
    for j, o in zip(run[:3], outs):
        assert submit(dec, j, o, stream=s) == [OK] * len(j.files)
    submitted_behind_the_delay = not b.query()
    assert submit(dec, run[3], outs[3], stream=s) == [OK] * len(run[3].files)    # blocks in WaitSlot
    assert b.query()                                                              # slot 0's batch is done, so the delay in front of it is
    dec.finish()
    lasted = held_for((a, b), target)
    print("delay: %.1f ms wanted, %.1f ms measured; three batches submitted behind it: %s" % (target, lasted, submitted_behind_the_delay))
    assert submitted_behind_the_delay
    for k, (j, o) in enumerate(zip(run, outs)):
        compare(j, o, "batch %d" % k)
    pin_one_lossy(run, outs, oracle_pixels)


# ---------------------------------------------------------------- 3. outputs are stream-ordered
def test_outputs_are_ordered_on_the_callers_stream(dec, jobs, oracle_pixels):
    """No finish(): a copy enqueued on the caller's stream behind the submit sees the finished pixels.  The stream is held, so a copy
    that was not ordered behind the decode would read the fill."""
    import torch
    run = [jobs[1], jobs[2], jobs[0]]     # (no one-group lossy frame: its LF pre-pass frees a temporary, which waits for the whole device)
    outs = [j.outputs() for j in run]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a, b = hold(s, HOLD_MS)
    for j, o in zip(run, outs):
        assert submit(dec, j, o, stream=s) == [OK] * len(j.files)
    with torch.cuda.stream(s):
        copies = [[t.clone() for t in o] for o in outs]
    held = not b.query()
    s.synchronize()
    assert held_for((a, b), HOLD_MS) and held      # the copies were enqueued while every output still held the fill
    for k, (j, c) in enumerate(zip(run, copies)):
        compare(j, c, "copy of batch %d" % k)
    pin_one_lossy(run, copies, oracle_pixels)
    dec.finish()


# ---------------------------------------------------------------- 4. "overlap" = 0
def test_one_stream_for_all_three_chains(dec, jobs, oracle_pixels):
    import torch
    assert dec.set_option("overlap", 0) == 1
    try:
        outs = [j.outputs() for j in jobs]
        torch.cuda.synchronize()
        for j, o in zip(jobs, outs):
            assert submit(dec, j, o) == [OK] * len(j.files)
        dec.finish()
    finally:
        dec.set_option("overlap", 1)
    for k, (j, o) in enumerate(zip(jobs, outs)):
        compare(j, o, "batch %d" % k)
    pin_one_lossy(jobs, outs, oracle_pixels)
    # and back: the same decoder, three streams again
    outs = [j.outputs() for j in jobs[:4]]
    torch.cuda.synchronize()
    for j, o in zip(jobs, outs):
        submit(dec, j, o)
    dec.finish()
    for k, (j, o) in enumerate(zip(jobs, outs)):
        compare(j, o, "batch %d, overlap on again" % k)


# ---------------------------------------------------------------- 5. statuses and the sticky error
def _with_bad_file(jobs, bad, bad_bytes):
    """[good, bad, good]: two files of the table around a file that fails."""
    a, b = jobs[3], jobs[1]
    return Job([a.files[0], bad, b.files[2]], [a.sizes[0], bad_bytes, b.sizes[2]], [a.want[0], None, b.want[2]],
               cases=[a.cases[0], None, b.cases[2]])


@pytest.fixture(scope="module")
def afv_files(oracle):
    """test_gpu_parity.test_afv_varblocks_are_refused_loudly: several groups / a one-group frame.  Both failures are found on the
    device, by lf_finish_kernel when it lays the varblocks out (the LF pre-pass of a one-group frame only decodes tokens)."""
    return {"groups": (oracle.encode(synth(520, 300, 3), mislabel_afv=True), 520 * 300 * 4),
            "one-group": (oracle.encode(synth(200, 150, 3), mislabel_afv=True), 200 * 150 * 4)}


@pytest.mark.parametrize("batches,which", [(3, "groups"), (4, "groups"), (3, "one-group"), (4, "one-group")])
def test_device_failure_of_an_older_batch_is_sticky(dec, jobs, afv_files, oracle_pixels, batches, which):
    """An AFV file's failure is found on the device, so every status at submit is Ok; finish() reports the older batch's failure
    with its text, while the last batch's statuses are all Ok.  Four batches: slot 0 is reused before finish(), and the failure
    is noted there."""
    import torch
    run = [_with_bad_file(jobs, *afv_files[which]), jobs[1], jobs[3], jobs[6]][:batches]
    outs = [j.outputs() for j in run]
    torch.cuda.synchronize()
    for j, o in zip(run, outs):
        assert submit(dec, j, o) == [OK] * len(j.files)
    name, st = dec.finish(raise_on_error=False)
    msg = dec.last_error
    assert name == "DecodeError" and st == [OK] * len(run[-1].files)      # the older batch's failure, the last batch's statuses
    assert "an earlier asynchronous batch failed" in msg and "AFV" in msg and "image 1" in msg, msg
    assert dec.finish() == ("Ok", [OK] * len(run[-1].files))              # reported once
    for k, (j, o) in enumerate(zip(run, outs)):
        compare(j, o, "batch %d" % k)
    pin_one_lossy(run, outs, oracle_pixels)


def test_device_failure_of_the_last_batch_is_its_own(dec, jobs, afv_files, oracle_pixels):
    """The same file in the most recent batch: its status and its text, nothing about older batches.  finish() raises by default;
    the batch's own failure is not a sticky one, so asking again gives the same answer."""
    import torch
    run = [jobs[0], _with_bad_file(jobs, *afv_files["groups"])]
    outs = [j.outputs() for j in run]
    torch.cuda.synchronize()
    for j, o in zip(run, outs):
        assert submit(dec, j, o) == [OK] * len(j.files)
    with pytest.raises(api.FormatError) as e:
        dec.finish()
    assert e.value.status == "DecodeError" and "AFV" in str(e.value) and "image 1" in str(e.value), str(e.value)
    name, st = dec.finish(raise_on_error=False)
    assert name == "DecodeError" and st == [OK, DECODE_ERROR, OK]
    assert "AFV" in dec.last_error and "image 1" in dec.last_error and "earlier" not in dec.last_error, dec.last_error
    for k, (j, o) in enumerate(zip(run, outs)):
        compare(j, o, "batch %d" % k)
    pin_one_lossy(run, outs, oracle_pixels)


def test_host_failure_is_there_at_submit(dec, jobs, oracle_pixels):
    """A truncated file fails in the host's parse: its status is there when the submit returns, nothing is written for it, and the rest
    of the batch and the later batches decode.  As the failure of an older batch it is sticky like one the device found."""
    import torch
    good = jobs[0].files[0]
    for batches in (3, 4):
        run = [_with_bad_file(jobs, good[:len(good) // 8], 16), jobs[5], jobs[2], jobs[0]][:batches]
        outs = [j.outputs() for j in run]
        torch.cuda.synchronize()
        st = submit(dec, run[0], outs[0], raise_on_error=False)      # (the call's own status is the truncated file's: it would raise)
        assert st[0] == OK and st[1] != OK and st[2] == OK, st
        for j, o in zip(run[1:], outs[1:]):
            assert submit(dec, j, o) == [OK] * len(j.files)
        name, last = dec.finish(raise_on_error=False)
        assert last == [OK] * len(run[-1].files)
        assert name == api.DECODER_STATUS[st[1]] and dec.last_error.startswith("an earlier asynchronous batch failed: "), (name, dec.last_error)
        assert len(dec.last_error) > len("an earlier asynchronous batch failed: ")
        assert dec.finish()[0] == "Ok"
        for k, (j, o) in enumerate(zip(run, outs)):
            compare(j, o, "batch %d" % k)
        assert (outs[0][1].cpu().numpy() == FILL).all()      # a file refused on the host is not written to
        pin_one_lossy(run, outs, oracle_pixels)


# ---------------------------------------------------------------- 6. while a batch is pending
def test_queries_while_a_batch_is_pending(dec, jobs, oracle_pixels):
    import torch
    job = jobs[0]                       # lossy RGBA: an "lf" plane and alpha groups
    outs = job.outputs()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a, b = hold(s, HOLD_MS)
    submit(dec, job, outs, stream=s)
    pending = not b.query()
    with pytest.raises(KeyError):
        dec.read_plane(0, "lf")
    assert dec.set_option("query_alpha_narrow_groups", 0) == -1
    assert dec.set_option("query_alpha_redo_groups", 0) == -1
    still_pending = not b.query()
    dec.finish()
    held_for((a, b), HOLD_MS)
    assert pending and still_pending        # the questions were asked while the pixel stages stood behind the delay
    h, w, _ = job.cases[0].shape
    assert dec.read_plane(0, "lf").size == ((h + 7) // 8) * ((w + 7) // 8)
    assert dec.set_option("query_alpha_narrow_groups", 0) >= 0 and dec.set_option("query_alpha_redo_groups", 0) >= 0
    compare(job, outs)
    pin_one_lossy([job], [outs], oracle_pixels)


# ---------------------------------------------------------------- 7. synchronous and asynchronous calls mixed
def test_mixing_synchronous_and_asynchronous_batches(dec, jobs, oracle_pixels):
    import torch
    dec.finish()                        # nothing decoded yet
    dec.finish()
    assert dec.finish() == ("Ok", [])
    run = [jobs[1], jobs[2], jobs[5], jobs[6]]      # (the two held batches: no one-group lossy frame, see test 3)
    outs = [j.outputs() for j in run]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a, b = hold(s, HOLD_MS)
    for j, o in zip(run[:2], outs):
        assert submit(dec, j, o, stream=s) == [OK] * len(j.files)
    was_held = not b.query()
    assert submit(dec, run[2], outs[2], stream=s, synchronize=True) == [OK] * len(run[2].files)   # its Finish waits for the two older ones
    assert dec.stage_totals()[1] == 3
    for k in range(3):                  # all three are complete when the synchronous call returns: no finish() in between
        compare(run[k], outs[k], "batch %d" % k)
    assert submit(dec, run[3], outs[3], stream=s) == [OK] * len(run[3].files)
    dec.finish()
    dec.finish()
    assert held_for((a, b), HOLD_MS) and was_held      # both asynchronous submits came back while the delay ran
    compare(run[3], outs[3], "batch 3")
    pin_one_lossy(run, outs, oracle_pixels)


# ---------------------------------------------------------------- the destructor waits for what is in flight
def test_close_with_batches_in_flight(jobs, oracle_pixels):
    """close() behind two submitted batches whose pixel stages have not started: the destructor waits for both before it frees the
    slots' memory and events, so the outputs are complete afterwards.  (It waits twice over - for every pending slot's `done`, then
    for the device - so this test holds the behaviour, not which of the two waits gives it.)"""
    import torch
    d = api.Decoder(0)
    run = [jobs[1], jobs[0]]            # (no one-group lossy frame, see test 3)
    outs = [j.outputs() for j in run]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a, b = hold(s, HOLD_MS)
    for j, o in zip(run, outs):
        submit(d, j, o, stream=s)
    in_flight = not b.query()
    d.close()
    assert in_flight and b.query()      # close() was called behind the delay and came back after it, i.e. after both batches
    torch.cuda.synchronize()
    for k, (j, o) in enumerate(zip(run, outs)):
        compare(j, o, "batch %d" % k)
    held_for((a, b), HOLD_MS)
    pin_one_lossy(run, outs, oracle_pixels)
