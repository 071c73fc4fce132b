"""The GPU inflate (csrc/bgzf_gpu.hip) against zlib on the designed streams of tests/inflatecases.py: every class A case through
both decoders (lanes, rounds), both sets of kernels (unshared, _shared) and both output layouts (256-aligned blocks, abutting
blocks), byte for byte; every stream zlib rejects, and the stated limit, must come back as an error from both decoders.
tests/test_cpu_inflate.py proves without a GPU that each case is what its name says."""
import pytest

from breakid_amd import capi
from tests import inflatecases as ic

pytestmark = pytest.mark.gpu

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _info():
    return capi.bgzf_info()


def _first_difference(got, want):
    n = min(len(got), len(want))
    for i in range(n):
        if got[i] != want[i]:
            return "first difference at offset %d: GPU %d, zlib %d" % (i, got[i], want[i])
    return "GPU gave %d bytes, zlib %d" % (len(got), len(want))


def _run_image(named, form_name, align):
    """named: [(label, Stream)]; one call; a list of what is wrong, each entry naming case, form and alignment"""
    img, offs = ic.bgzf_image([s for _, s in named])
    for (label, s), off in zip(named, offs):
        assert s.in_align is None or off & 3 == s.in_align, label
    rc, out, err = capi.bgzf_inflate_form(img + EOF_BLOCK, ic.FORMS[form_name], align)
    where = "form %s, out_align %d" % (form_name, align)
    if rc != 0:
        if len(named) == 1:
            return ["%s: %s: rc %d (%s)" % (named[0][0], where, rc, err)]
        bad = []  # one error flag per call: find the cases by running them alone
        for one in named:
            bad += _run_image([one], form_name, align)
        return bad or ["the whole image: %s: rc %d (%s), but every case alone is right" % (where, rc, err)]
    bad, at = [], 0
    for label, s in named:
        want = ic.zlib_reference(s)
        got = out[at:at + s.isize]
        at += s.isize
        if got != want:
            bad.append("%s: %s: %s" % (label, where, _first_difference(got, want)))
    assert at == len(out)
    return bad


@pytest.mark.parametrize("family", ic.FAMILIES)
def test_streams_zlib_accepts_in_every_form_and_alignment(family):
    named = [("%s[%d]" % (c.name, k), s) for c in ic.cases(_info()) if c.cls == "A" and c.family == family for k, s in enumerate(c.streams)]
    assert named
    bad = []
    for form_name in ic.FORMS:
        for align in ic.ALIGNS:
            bad += _run_image(named, form_name, align)
    assert not bad, "\n".join(bad)


def _rejected_cases():
    return [c for c in ic.cases() if c.cls in ("B", "D")]  # (the names; the streams are rebuilt from the build's constants below)


@pytest.mark.parametrize("name", [c.name for c in _rejected_cases()])
def test_streams_that_must_be_reported(name):
    """class B: zlib rejects the stream (or it does not give ISIZE bytes); class D: more deflate blocks than decode_wave takes.
    One error flag per call, so one stream per call; rc != 0, never bytes"""
    case = [c for c in ic.cases(_info()) if c.name == name and c.cls in ("B", "D")]
    assert len(case) == 1 and len(case[0].streams) == 1
    img, _ = ic.bgzf_image(case[0].streams)
    for form_name in ("lanes", "rounds"):
        rc, out, err = capi.bgzf_inflate_form(img + EOF_BLOCK, ic.FORMS[form_name], 256)
        assert rc != 0 and out is None, "%s: form %s: accepted (%d bytes)" % (name, form_name, len(out or b""))
        assert "inflate failed" in err, (name, form_name, err)


def test_no_stream_is_tolerated_that_zlib_rejects():
    """class C of the plan - an incomplete code set that zlib rejects and the kernel accepted - is empty: build_tables rejects it"""
    assert not [c for c in ic.cases(_info()) if c.cls == "C"]


def test_more_blocks_than_one_launch_pair_takes():
    """BGZF_BATCH_BLOCKS + 1 blocks: the second launch pair starts at `first` = BGZF_BATCH_BLOCKS and reuses the token slab"""
    info = _info()
    img, streams = ic.batch_image(info)
    n = info["BGZF_BATCH_BLOCKS"] + 1
    assert len(streams) == n
    want = b"".join(ic.zlib_reference(s) for s in streams)
    for form_name in ("lanes", "lanes_shared"):
        rc, out, err = capi.bgzf_inflate_form(img + EOF_BLOCK, ic.FORMS[form_name], 256)
        assert rc == 0, (form_name, err)
        if out != want:
            at = 0
            for i, s in enumerate(streams):
                w = ic.zlib_reference(s)
                assert out[at:at + len(w)] == w, "block %d of %d: form %s: %s" % (i, n, form_name, _first_difference(out[at:at + len(w)], w))
                at += len(w)
            assert False, "form %s: the blocks agree but the whole does not" % form_name


def test_the_hook_refuses_other_forms_and_alignments():
    img, _ = ic.bgzf_image([s for c in ic.cases(_info()) if c.name == "stream_ends_inside_lane_0" for s in c.streams])
    for form, align in ((4, 256), (-1, 256), (0, 4), (0, 0), (1, 255)):
        rc, out, err = capi.bgzf_inflate_form(img + EOF_BLOCK, form, align)
        assert rc == -1 and out is None and "bk_debug_bgzf_inflate_form" in err, (form, align, rc, err)
