"""How the edge goldens (tests/golden/nsx_edges_golden.npz, agc_edges_golden.npz) hold the output of a long run, shared
by the two runs files, the golden writers and the tests."""
import ctypes as C
import hashlib

import numpy as np

# Outputs of a long edge run do not fit the golden in full (noise does not compress): the golden keeps every sample of
# the 20 frames from each snapshot on, and a sha256 per block of 50 frames of the whole run.
BLOCK, KEEP = 50, 20


def kept_frames(spec):
    if spec["frames"] <= 120:
        return list(range(spec["frames"]))
    return sorted({f for s in spec["snaps"] for f in range(s, min(s + KEEP, spec["frames"]))})


def pack_outputs(spec, out):
    """out: int16 [frames][samples of a frame].  Returns (kept samples, block digests uint8 [blocks][32])."""
    out = np.ascontiguousarray(out, np.int16).reshape(spec["frames"], -1)
    digests = [np.frombuffer(hashlib.sha256(out[a:a + BLOCK].tobytes()).digest(), np.uint8) for a in range(0, spec["frames"], BLOCK)]
    return out[kept_frames(spec)].reshape(-1), np.stack(digests)


def compare_outputs(spec, out, keep, blocks):
    """None when `out` equals what pack_outputs stored, else a message that names the first differing frame or block."""
    got_keep, got_blocks = pack_outputs(spec, out)
    if got_keep.shape != keep.shape or got_blocks.shape != blocks.shape:
        return "output sizes differ: %r, %r against %r, %r" % (got_keep.shape, got_blocks.shape, keep.shape, blocks.shape)
    bad = [k for k in range(len(blocks)) if not np.array_equal(got_blocks[k], blocks[k])]
    per = got_keep.size // len(kept_frames(spec))
    diff = np.nonzero(got_keep != keep)[0]
    if diff.size:
        return "frame %d, sample %d differs; differing blocks of %d frames: %r" % (kept_frames(spec)[diff[0] // per], diff[0] % per, BLOCK, bad)
    if bad:
        return "the output differs in frames %d..%d (sha256 of the block); differing blocks: %r" % (
            bad[0] * BLOCK, min(bad[0] * BLOCK + BLOCK, spec["frames"]) - 1, bad)
    return None


# A snapshot is one array: the bytes of the project's flat state struct (AspNsxState, AspAgcState) filled field by field
# from the reference's instance -- a zip entry per field and snapshot would cost more than the fields themselves.
def pack_state(cls, fields):
    """fields: {name: array} as state_dict() gives it.  Returns the struct's bytes as uint8 (padding zero)."""
    st = cls()
    for name, v in fields.items():
        v = np.ascontiguousarray(v)
        C.memmove(C.addressof(st) + getattr(cls, name).offset, v.ctypes.data, v.nbytes)
    return np.frombuffer(bytes(st), np.uint8).copy()


def unpack_state(cls, packed):
    return cls.from_buffer_copy(np.ascontiguousarray(packed, np.uint8).tobytes())
