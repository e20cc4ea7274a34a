"""What the host modules of the data pipeline share: the op codes of the augmentation kernels and the counted call into the library.

Op codes.  The world transforms, the local steps and the world dropout each take their ops as up to 16 codes of 4 bits in one int64, first op
in the lowest bits (csrc/augment.h: aug_code).  `OP_CODES` is the one statement of which draw name means which code of which kernel family;
the switches of csrc/augment.hip (world) and the enums of csrc/augment_local.hip (local, drop) are its device side.
"""
from . import _lib as L

# draw name -> (kind, code); kind: "world" sv_world_transform_*, "local" sv_local_transform_*, "drop" sv_world_frustum_dropout
OP_CODES = {
    "flip_x": ("world", 1), "flip_y": ("world", 2), "rotation": ("world", 3), "scaling": ("world", 4),
    "translation_x": ("world", 5), "translation_y": ("world", 6), "translation_z": ("world", 7),
    "local_translation_x": ("local", 1), "local_translation_y": ("local", 2), "local_translation_z": ("local", 3),
    "local_rotation": ("local", 4), "local_scaling": ("local", 5),
    "local_dropout_top": ("local", 6), "local_dropout_bottom": ("local", 7), "local_dropout_left": ("local", 8), "local_dropout_right": ("local", 9),
    "world_dropout_top": ("drop", 1), "world_dropout_bottom": ("drop", 2), "world_dropout_left": ("drop", 3), "world_dropout_right": ("drop", 4),
}


def codes_of(kind):
    """name -> code for one kind, in table order."""
    return {name: code for name, (k, code) in OP_CODES.items() if k == kind}


def op_kind(name):
    """The kind of a draw name; None for a draw that is no coded op (object_scaling, gt_sampling)."""
    return OP_CODES[name][0] if name in OP_CODES else None


def pack_codes(names, kind):
    """The int64 a kernel of `kind` takes for `names` in order; a name of another kind is a KeyError."""
    assert len(names) <= 16
    table, packed = codes_of(kind), 0
    for i, name in enumerate(names):
        packed |= table[name] << (4 * i)
    return packed


class Counted:
    """Library calls and blocking device -> host reads, counted in a dict of the owner's own.  A host module makes one and publishes
    `counters` as COUNTERS, `reset` as reset_counters, and `call` / `read` / `host_ints` under their own names."""

    def __init__(self):
        self.counters = {"library_calls": 0, "host_reads": 0}

    def reset(self):
        self.counters.update(library_calls=0, host_reads=0)

    def call(self, name, *args):
        """One launch through the binding layer, counted."""
        self.counters["library_calls"] += 1
        L.launch(name, *args)

    def read(self, t):
        """One blocking device -> host read, counted."""
        self.counters["host_reads"] += 1
        return t.cpu().numpy()

    def host_ints(self, tensors):
        """One blocking device -> host read, counted (checks parked on the stream ride on it)."""
        self.counters["host_reads"] += 1
        return L.host_ints(tensors)
