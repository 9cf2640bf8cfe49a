"""What every object that owns a handle of the C ABI does the same way: the way to the loaded library, the create call,
the checked call, the refusal once it is closed, and close() / __del__ / the context manager.

    class SpeckleFilter(Handle):
        _destroy = "mrcal_amd_speckle_filter_destroy"
        def __init__(self, shape):
            self._create("filter_speckles()", "mrcal_amd_speckle_filter_create", W, H)
        def filter(self, ...):
            self._open()                                     # "this SpeckleFilter has been closed"
            self._call("filter_speckles()", "mrcal_amd_speckle_filter_apply", ...)      # handle first

The signatures are _cabi.SIGNATURES, applied when the library was loaded.
"""


def _libs():
    """(the loaded library, its Api): the ONE gateway of the handle-owning objects and their modules' functions. Nothing
    touches the library before it is called, which is what the tests of the refusals replace it for"""
    from . import _lib, _api
    return _lib, _api


def _failed(what, error=Exception):
    return error(f"{what} failed:" + _libs()[1]._last_error())


class Handle:
    _destroy = None         # the name of the destroy function
    _error = Exception      # what a failed call raises
    handle = None

    def _function(self, name):
        return getattr(_libs()[0].lib, name)

    def _create(self, what, name, *args):
        """self.handle = name(*args); NULL raises '<what> failed:' + the library's last error"""
        self.handle = self._function(name)(*args) or None
        if self.handle is None:
            raise _failed(what, self._error)

    def _open(self):
        if self.handle is None:
            raise self._error(f"this {type(self).__name__} has been closed")

    def _call(self, what, name, *args):
        """name(handle, *args), which returns false when it fails"""
        self._open()
        if not self._function(name)(self.handle, *args):
            raise _failed(what, self._error)

    def close(self):
        handle, self.handle = self.handle, None
        if handle:
            self._function(self._destroy)(handle)

    def __del__(self):
        try:    self.close()
        except Exception: pass

    def __enter__(self): return self
    def __exit__(self, *a): self.close()
