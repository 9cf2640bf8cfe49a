"""mrcal_amd/_handle.py, the base of every object that owns a handle of the C ABI, against a library that only records
what is called: creation, the checked call, the refusal once closed, close() and __del__. No GPU, no device work."""
import numpy as np
import pytest


class FakeLibrary:
    """stands where _handle._libs() is: every function of .lib records its call and returns what `returns` says (1
    otherwise: a handle, or true)"""
    def __init__(self, **returns):
        self.calls, self.returns = [], returns
        self.lib = self

    def __getattr__(self, name):
        def function(*args):
            self.calls.append((name,) + args)
            return self.returns.get(name, 1)
        return function

    def _last_error(self):
        return " the library's reason"

    def __call__(self):
        return self, self

    def called(self, name):
        return [c for c in self.calls if c[0] == name]


@pytest.fixture
def fake(amd, monkeypatch):
    def install(**returns):
        library = FakeLibrary(**returns)
        monkeypatch.setattr(amd._handle, "_libs", library)
        return library
    return install


def test_create_that_returns_null_raises_the_class_own_message(amd, fake):
    from mrcal_amd.resident import Problem
    library = fake(mrcal_amd_speckle_filter_create=0, mrcal_amd_equalizer_create=None)
    f = amd.SpeckleFilter.__new__(amd.SpeckleFilter)
    with pytest.raises(Exception, match="^filter_speckles\\(\\) failed: the library's reason$") as e:
        f.__init__((20, 30))
    assert e.type is Exception and f.handle is None
    assert library.called("mrcal_amd_speckle_filter_create") == [("mrcal_amd_speckle_filter_create", 30, 20)]
    q = amd.ImageEqualizer.__new__(amd.ImageEqualizer)
    with pytest.raises(Exception, match="^equalize\\(\\) failed: the library's reason$"):
        q.__init__((20, 30), np.uint8)
    assert q.handle is None
    # ... and nothing is there to destroy
    f.close(); q.close(); f.__del__()
    assert not library.called("mrcal_amd_speckle_filter_destroy") and not library.called("mrcal_amd_equalizer_destroy")
    # Problem says RuntimeError
    p = Problem.__new__(Problem)
    library.returns["mrcal_amd_problem_create_sharded"] = 0
    with pytest.raises(RuntimeError, match="^mrcal_amd_problem_create\\(\\) failed: the library's reason$"):
        p._create("mrcal_amd_problem_create()", "mrcal_amd_problem_create_sharded")
    assert p.handle is None


def test_close_destroys_once(amd, fake):
    library = fake(mrcal_amd_speckle_filter_create=77)
    with amd.SpeckleFilter((20, 30)) as f:
        assert f.handle == 77
    assert f.handle is None
    assert library.called("mrcal_amd_speckle_filter_destroy") == [("mrcal_amd_speckle_filter_destroy", 77)]
    f.close(); f.close(); f.__del__()
    assert len(library.called("mrcal_amd_speckle_filter_destroy")) == 1
    # an object made by hand whose planted handle was taken back: nothing to destroy either
    g = amd.SpeckleFilter.__new__(amd.SpeckleFilter)
    g.handle = 1
    g.handle = None
    g.close(); g.__del__()
    assert len(library.called("mrcal_amd_speckle_filter_destroy")) == 1


def test_del_of_an_object_whose_init_raised_before_the_handle(amd, fake):
    library = fake()
    f = amd.SpeckleFilter.__new__(amd.SpeckleFilter)
    with pytest.raises(Exception, match="shape must be"):
        f.__init__((20, 30, 3))
    e = amd.ImageEqualizer.__new__(amd.ImageEqualizer)
    with pytest.raises(Exception, match="images are uint8 or uint16"):
        e.__init__((20, 30), np.float32)
    f.__del__(); e.__del__()
    assert library.calls == []


def test_calls_after_close_are_refused(amd, fake):
    from mrcal_amd.resident import Problem
    library = fake()
    a = np.zeros((20, 30), dtype=np.int16)
    f = amd.SpeckleFilter((20, 30))
    e = amd.ImageEqualizer((20, 30), np.uint8, 'stretch')
    t = amd.Triangulation.__new__(amd.Triangulation)
    p = Problem.__new__(Problem)
    t.handle = p.handle = 5
    for x in (f, e, t, p):
        x.close()
    Ncalls = len(library.calls)
    with pytest.raises(Exception, match="^this SpeckleFilter has been closed$"):
        f.filter(a, new_value=-16, max_speckle_size=10, max_diff=16)
    with pytest.raises(Exception, match="^this SpeckleFilter has been closed$"):
        f.milliseconds()
    with pytest.raises(Exception, match="^this ImageEqualizer has been closed$"):
        e.apply(a.astype(np.uint8))
    with pytest.raises(Exception, match="^this Triangulation has been closed$"):
        t.triangulate(np.zeros((2, 2)))
    with pytest.raises(RuntimeError, match="^this Problem has been closed$"):
        p.evaluate()
    with pytest.raises(RuntimeError, match="^this Problem has been closed$"):
        p.synchronize()
    assert len(library.calls) == Ncalls         # (refused before anything was called)


def test_failed_call_raises_what_the_class_raises(amd, fake):
    from mrcal_amd.resident import Problem
    library = fake(mrcal_amd_problem_evaluate=False, mrcal_amd_speckle_filter_milliseconds=False)
    p = Problem.__new__(Problem)
    p.handle = 5
    with pytest.raises(RuntimeError, match="^evaluate failed: the library's reason$"):
        p.evaluate()
    assert library.called("mrcal_amd_problem_evaluate") == [("mrcal_amd_problem_evaluate", 5, True, True)]
    p.handle = None
    with amd.SpeckleFilter((20, 30)) as f:
        with pytest.raises(Exception, match="^filter_speckles\\(\\) failed: the library's reason$") as e:
            f.milliseconds()
        assert e.type is Exception
