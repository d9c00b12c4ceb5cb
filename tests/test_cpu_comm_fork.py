"""``DirectComm.__del__`` destroys its communicator only in the process that created it: a forked child that finalises an
inherited copy (multiprocessing's Manager server collecting the parent's garbage) must leave the handle alone."""
import ctypes
import os


class _Lib:
    def __init__(self):
        self.destroyed = []

    def vlb_comm_destroy(self, h):
        self.destroyed.append(h.value)
        return 0


def _comm(pid, handle=0x1000):
    from phantom_vlb_amd.parallel_native import DirectComm
    c = DirectComm.__new__(DirectComm)
    c._h, c._pid = ctypes.c_void_p(handle), pid
    return c


def test_only_the_creating_process_destroys(monkeypatch):
    from phantom_vlb_amd import parallel_native
    fake = _Lib()
    monkeypatch.setattr(parallel_native, "lib", fake)
    mine = _comm(os.getpid(), 0x1000)
    mine.__del__()
    assert fake.destroyed == [0x1000] and mine._h is None
    mine.__del__()                                   # a second finalisation finds nothing
    assert fake.destroyed == [0x1000]
    inherited = _comm(os.getpid() + 1, 0x2000)       # as a forked child sees its parent's object
    inherited.__del__()
    assert fake.destroyed == [0x1000] and inherited._h is None
    del mine, inherited
