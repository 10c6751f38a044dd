"""CPU: renderer.UncheckedFrames, the record of which workspace slices hold frames that no stats() has read yet — which slices
a call must reset before it chains onto the others (GsrOptions.keep_flags), and which ones stats() reads."""


def test_a_slice_starts_a_new_record_unless_it_holds_unchecked_frames():
    from gsr_amd.renderer import UncheckedFrames

    u = UncheckedFrames()
    assert u.slices == 0 and list(u.to_reset(3)) == []          # every slice fresh: the batch starts new records
    u.wrote(1)                                                   # enqueue(): slice 0
    assert list(u.to_reset(1)) == []                             # the next single frame adds to its record
    assert list(u.to_reset(3)) == [1, 2]                         # a batch of three chains onto slice 0: slices 1, 2 reset first
    u.wrote(3)
    assert u.slices == 3 and list(u.to_reset(2)) == [] and list(u.to_reset(3)) == []
    u.wrote(2)                                                   # a smaller batch later: the record still covers three slices
    assert u.slices == 3 and list(u.to_reset(4)) == [3]


def test_stats_reads_the_unchecked_slices_and_starts_over():
    from gsr_amd.renderer import UncheckedFrames

    u = UncheckedFrames()
    assert u.read() == 1                                         # nothing unchecked: slice 0's last frame, once more
    u.wrote(3)
    assert u.read() == 3 and u.slices == 0                       # every slice that holds unchecked frames, then a new record
    assert u.read() == 1


def test_a_reported_batch_leaves_nothing_for_the_next_chain():
    """A batch over three slices is read (its overflow reported), then a single frame and a batch of three: the batch chains onto
    the single frame in slice 0 and resets slices 1 and 2 — their record was reported already."""
    from gsr_amd.renderer import UncheckedFrames

    u = UncheckedFrames()
    u.wrote(3)
    assert u.read() == 3
    u.wrote(1)
    assert list(u.to_reset(3)) == [1, 2]
    u.wrote(3)
    assert u.read() == 3


def test_an_empty_shard_leaves_the_frames_before_it_to_be_read():
    from gsr_amd.renderer import UncheckedFrames

    u = UncheckedFrames()
    u.wrote(2)
    u.wrote(0)                                                   # a shard without tile rows: no kernel ran
    assert u.empty and u.slices == 2
    assert u.read() == 2                                         # the unchecked frames before it are still read
    assert u.empty and u.read() == 0                             # and nothing more: the shard's own counters are zeros
    u.wrote(1)
    assert not u.empty and list(u.to_reset(1)) == [] and u.read() == 1


def test_a_single_view_chains_onto_unchecked_frames_with_a_copy_of_the_options():
    """Rasterizer._chained, the one statement of the rule every single-view call follows: the caller's options as they are while
    slice 0 holds nothing unchecked or the flag is set already, else a copy with keep_flags = 1 — never a write to the caller's."""
    from gsr_amd.renderer import Rasterizer, UncheckedFrames, make_options

    R = Rasterizer.__new__(Rasterizer)
    R.unchecked = UncheckedFrames()
    plain, kept = make_options(depth_sort_passes=3), make_options(keep_flags=True)
    assert R._chained(plain) is plain and R._chained(kept) is kept      # nothing unchecked
    R.unchecked.wrote(0)                                                # an empty shard leaves nothing to chain onto
    assert R._chained(plain) is plain
    R.unchecked.wrote(1)
    o = R._chained(plain)
    assert o is not plain and o.keep_flags == 1 and plain.keep_flags == 0
    assert bytes(o) != bytes(plain)
    o.keep_flags = 0
    assert bytes(o) == bytes(plain)                                      # every other field is the caller's
    assert R._chained(kept) is kept                                      # the flag is set already
    R.unchecked.read()
    assert R._chained(plain) is plain                                    # stats() has read the record
