"""NativeComm hands the library real events: a ``torch.cuda.Event`` has no HIP event behind it until its first record, and a null
``done_event`` makes ``bsclip_allgather_*`` / ``bsclip_allreduce_grads`` record nothing, so that a consumer's ``wait_event(done)``
orders nothing behind the collective (it then reads the gathered rows while the producer's stream is still writing them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_done_event_exists_when_the_library_gets_it():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip.dist import NativeComm
    comm = NativeComm(rank=0, world=1)
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ready, done = comm._events()
        assert ready.cuda_event != 0 and done.cuda_event != 0
        z = torch.arange(256 * 8, dtype=torch.float32, device="cuda").view(256, 8)
        seen = []
        real = comm._ev
        comm._ev = lambda e: (seen.append(e.cuda_event), real(e))[1]
        gathered, done = comm.all_gather(z)
        assert len(seen) == 2 and all(seen), seen            # neither handle the entry point received was null
        done.synchronize()                                    # the host waits for the collective alone
        assert done.query() and torch.equal(gathered, z)
    finally:
        comm.close()
