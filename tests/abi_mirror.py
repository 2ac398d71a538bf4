"""The check that the CPU tests of the prediction batches share: a svt_hip_*_layout(what, field) entry of the library against the
ctypes structs of svt_av1_psyex_amd.abi that mirror its header.  A plain helper module, not a conftest."""
import ctypes as C

from svt_av1_psyex_amd import api

NONE = C.c_size_t(-1).value  # what a layout entry answers outside its tables


def check_layout(entry, structs, only=None, multiple_of_8=False):
    """`entry` names the layout function, `structs` are the mirrors in the order of its `what`.  For every struct (or for the indices in `only`,
    where a file checks some of them): the size at field -1, every field's offset in order and NONE one past the last field, so that no member is
    left out of the mirror; then NONE one past the last struct and at what = -1.  multiple_of_8: every size is a multiple of 8 as well."""
    f = getattr(api.lib(), entry)
    f.restype = C.c_size_t
    for what in range(len(structs)) if only is None else only:
        t = structs[what]
        assert f(what, -1) == C.sizeof(t), t.__name__
        for i, (name, *_) in enumerate(t._fields_):
            assert f(what, i) == getattr(t, name).offset, (t.__name__, name)
        assert f(what, len(t._fields_)) == NONE, t.__name__
        if multiple_of_8:
            assert C.sizeof(t) % 8 == 0, t.__name__
    assert f(len(structs), -1) == NONE and f(-1, -1) == NONE
