"""The serial core of the device's BGZF encoder (kmers_amd/csrc/kmx_bgzf_encode.h) on the host, under a sanitizer: tests/cpp/
bgzf_encode_check.cpp is compiled with -fsanitize=address,undefined (without, where the compiler has no sanitizer runtime) and run as a
child process over the corpus of tests/bgzf_deflate_cases.py at block sizes 65280, 9000 and 256.  It codes every block in the wave's
step semantics, decodes it again with the project's host decoder and writes the images; here every image is held to zlib: gzip's
bytes, the walk, every block's verdict with CRC, the bound.  The size conditions are settled here too: the size is a function of the
text, so what holds for the host model holds for the device, which the GPU test holds to these bytes.  CPU only; nothing is loaded
into Python.

The host model's figures (profiles/bgzf_deflate_ratio.txt): text (e) 326045 bytes = 1.0430 of zlib level 1, 1.0726 of level 6,
0.9428 of Z_HUFFMAN_ONLY; text (f) 29076 bytes = 0.8223 of level 1, 1.1704 of level 6, 0.4692 of Z_HUFFMAN_ONLY; text (c) 134 bytes."""
import pytest

from tests import bgzf_deflate_cases as K
from tests import bgzf_np as B

SIZES = (65280, 9000, 256)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bgzf_encode")
    exe, sanitized = K.compile_host(tmp)
    ents = K.entries(SIZES)
    return ents, K.host_images(exe, ents, tmp), sanitized


def test_host_encoder_images_are_zlibs_text_under_sanitizer(model):
    ents, images, sanitized = model
    assert len(ents) == 3 * 16
    for (name, bb, _, text), (image, n_stored, _) in zip(ents, images):
        bo, _ = K.check_image(image, text, bb)
        assert sum(1 for b in range(len(bo) - 2) if B.first_btype(image[int(bo[b]):int(bo[b + 1])]) == 0) == n_stored, name
    if not sanitized:
        pytest.skip("the compiler has no sanitizer runtime here: the check ran and passed without -fsanitize=address,undefined")


def test_corpus_exercises_what_it_says(model):
    ents, images, _ = model
    by = {name: (text, image, n_stored, n_deflate) for (name, _, _, text), (image, n_stored, n_deflate) in zip(ents, images)}
    assert by["a_empty@65280"][1] == B.EOF_MARKER
    # (d) every block falls back to stored; (g) the only repeat lies 35000 back, so nothing is gained and the block is stored
    assert by["d_random@65280"][2] == 4 and by["g_far@65280"][2] == 1
    # (b) the cut: one block, and a second of one byte
    assert len(B.walk(by["b_exact_65280@65280"][1])[0]) - 1 == 2 and len(B.walk(by["b_plus1_65280@65280"][1])[0]) - 1 == 3
    # (i) more tokens than the buffer holds: several DEFLATE blocks inside the one BGZF block
    assert by["i_four_letters@65280"][2] == 0 and by["i_four_letters@65280"][3] >= 2
    # (h) dynamic blocks whose last match ends with the text / 3 bytes before it: the table's candidate at distance 117 is coded
    # (distance symbol 13; a literal-only coding, or one with the runs of the filler alone, has no such code)
    assert by["h_run_at_end@65280"][2] == 0 and by["h_match_then_3@65280"][2] == 0
    lit, dist = B.dynamic_code_lengths(by["h_match_then_3@65280"][1][:-28])
    assert len(dist) >= 14 and dist[13] > 0 and dist[6] > 0 and dist[5] > 0 and all(lit[c] > 0 for c in b"xyz")
    # (g), built: the candidate 33012 back is in the table when the word comes again (far_candidate_text asserts it) and is refused.
    # The block is dynamic, so its tokens are what zlib reads: a coder without the distance check writes distance 33012 - 32768 here
    # and the block's CRC fails (tried once with the check taken out of the header: status 14 on this text alone).
    text, image, n_stored, _ = by["g_far_candidate@65280"]
    assert n_stored == 0 and text[K.FAR_AT:K.FAR_AT + 12] == K.FAR_WORD
    # (j) no match: ten bytes are stored; the 256-byte pieces of (d) hold no match either and are stored -- the one-distance-code form
    # of a dynamic block with no match is what the pieces of (i) at 256 take where they hold none
    assert by["j_no_match@65280"][2] == 1
    text, image = by["i_four_letters@256"][:2]
    bo = B.walk(image)[0]
    lone = 0
    for b in range(len(bo) - 2):
        blk = image[int(bo[b]):int(bo[b + 1])]
        if B.first_btype(blk) == 2:
            lit, dist = B.dynamic_code_lengths(blk)
            assert lit[256] > 0
            lone += dist == [1]
    assert lone > 0


def test_stored_flag_is_zlibs_level_0(tmp_path):
    exe, _ = K.compile_host(tmp_path)
    ents = [(name, bb, K.STORED, t) for name, bb, _, t in K.entries((65280, 9000)) if name.split("_")[0] in "abdeg"]
    assert len(ents) >= 16
    for (name, bb, _, text), (image, n_stored, _) in zip(ents, K.host_images(exe, ents, tmp_path, "stored")):
        assert image == B.write(text, 0, bb), name
        assert n_stored == (len(text) + bb - 1) // bb and len(image) == K.bound(len(text), bb)


def test_sizes(model):
    ents, images, _ = model
    by = {name: (text, image) for (name, _, _, text), (image, _, _) in zip(ents, images)}
    # (c): at most 65 literals and 254 matches of 258 under a code of a handful of symbols
    assert len(by["c_one_byte@65280"][1]) < 1024
    for name in ("e_fastq", "f_illumina"):
        text, image = by[name + "@65280"]
        huff, l1, l6 = K.huffman_only_size(text), len(B.write(text, 1, 65280)), len(B.write(text, 6, 65280))
        print(f"{name}: text {len(text)} image {len(image)} huffman-only {huff} level 1 {l1} ({len(image) / l1:.4f}) level 6 {l6} ({len(image) / l6:.4f})")
        assert len(image) <= huff, name                                  # matches must pay for the headers: no margin
        assert len(image) <= K.RATIO_BOUND_L1[name] * l1, name          # the measured ratio rounded up to the next 0.05
