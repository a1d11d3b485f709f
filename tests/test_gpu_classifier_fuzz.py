"""-m gpu: fixed seeds of the classifier parity hunt (scripts/fuzz_classifier.py): every part of the device classifier against its
plain-loop host statement, byte for byte, on repeat-ridden references, random search parameters, mixed read lengths, reads drawn
several times, planted events on both strands, junction reads and bytes outside ACGTN, with random arguments of every part.
tests/test_classifier_fuzz_cpu.py asserts, without a GPU, what these very seeds hold.

Measured on the MI355X, seconds per block of four seeds at 1 500 reads a seed, input generation, host statements and the CPU
containment included: low 0.75, wide 1.09, default_parameters 1.53, multi_chromosome 1.18, outside_acgtn 1.10.  The hunt has found
no difference so far (508 campaign seeds, profiles/variant/fuzz_classifier.txt): no seed here is a regression seed yet."""
import pytest

from scripts import fuzz_classifier

pytestmark = pytest.mark.gpu

N_READS = 1500
# one block per stream; every stream holds a seed whose boxed count exceeds two scan / sort blocks (the first of each list)
STREAMS = {
    "low": [1001, 1009, 1011, 1013],                                  # random parameters (-x <= 4); 1011: max_listed 0; 1013: two chromosomes
    "wide": [200004, 200018, 200007, 200028],                         # -x up to 6, more insert sizes; 200028: three chromosomes
    "default_parameters": [300003, 300004, 300008, 300002],           # Pindel's default search parameters; 300003: 36-base reads
    "multi_chromosome": [400011, 400023, 400000, 400007],             # always two or three chromosomes: junction reads, -I
    "outside_acgtn": [600026, 600027, 600000, 600006],                # bytes outside ACGTN in one read in twelve; 600027: 24-base reads
}


@pytest.mark.parametrize("stream", sorted(STREAMS))
def test_classifier_fuzz_block(stream):
    for seed in STREAMS[stream]:
        assert fuzz_classifier.one_iteration(seed, N_READS, verbose=False), seed
        assert seed not in fuzz_classifier.SKIPPED, f"seed {seed}: the library rejects its parameters"
