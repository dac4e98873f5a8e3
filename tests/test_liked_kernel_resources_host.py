"""CPU: the resources of the liked-sum kernels (prep.hip), read from the built library.

query_liked_kernel<DT, W> and query_liked_vec_kernel<DT, W> are one template each for the
unweighted and the weighted sum. The merge must cost the unweighted instantiations nothing: no
scratch, no spills, and the chunk form's LDS weight array only where W is true -- 4096 bytes of
LDS (row ids and norms of 256 staged rows) unweighted, 6144 weighted, none in the element form.
Metadata notes only (test_kernel_resources_host.py's reader), no instruction text."""
import os
import re

from robot_ebert_amd import _lib
from test_kernel_resources_host import READELF, _gfx950_code_objects, _kernels


def test_liked_sum_kernels_resources(tmp_path):
    _lib.load()
    assert os.path.exists(READELF), READELF
    found = {}
    for i, image in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        elf = tmp_path / f"co{i}.elf"
        elf.write_bytes(image)
        for name, k in _kernels(str(elf)).items():
            # <DT, W> as mangled: ILi.ELb.EE
            m = re.match(r"_ZN3ebt\d+(query_liked(?:_vec)?_kernel)ILi([0-3])ELb([01])EE", name)
            if m:
                found[(m.group(1), int(m.group(2)), m.group(3) == "1")] = k
    want = {(form, dt, w) for form in ("query_liked_kernel", "query_liked_vec_kernel")
            for dt in range(4) for w in (False, True)}
    assert set(found) == want, sorted(found)
    for (form, dt, w), k in sorted(found.items()):
        print(form, dt, w, k)
        assert k["private_segment_fixed_size"] == 0, (form, dt, w, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (form, dt, w, k)
        lds = 0 if form == "query_liked_kernel" else (6144 if w else 4096)
        assert k["group_segment_fixed_size"] == lds, (form, dt, w, k)
