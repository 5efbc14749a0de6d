"""The blocks and tables of tests/test_gpu_ransac_cert_table.py are what its docstring promises - certified blocks at
every size, zero planes that win from a later hypothesis, the draw of position n - checked without a GPU, by the NumPy
model of the certificate and by the oracle (about 330 blocks under three tables)."""

from tests import test_gpu_ransac_cert_table as ct


def test_blocks_are_what_they_claim_by_the_oracle():
    ct.check_blocks(ct._oracle)
