"""The directed blocks of tests/test_gpu_ransac_cert_exit.py are what their names promise - the best count of group 0,
the certificate by the NumPy model, the oracle's winner - checked without a GPU, so that the GPU test cannot silently
test nothing on a machine where nobody looks at it.  The oracle runs on the 1 500 leading blocks of each of the four
tables (a few seconds each)."""

from tests import test_gpu_ransac_cert_exit as ce


def test_directed_blocks_are_what_they_claim_by_the_oracle():
    ce.check_directed_blocks(ce._oracle)
