"""hvcoord_t / hvcoord_init (reference src/share/hybvcoord_mod.F90:18-171): hybrid vertical coordinate read from the
ascii files the reference's namelists name (test/dcmip1-1/dcmip1-1.nl: vcoord/acme-72{m,i}.ascii).  The two data
files are shipped as data under transport_se_amd/data/vcoord/.  Any level count is read (the reference's plev is a build setting:
dimensions_mod.F90:27); the library that runs it must be built for the same count (_lib.lib(nlev=...), tse_nlev()).
The reference's other grids (test/dcmip1-1/dcmip1-1.nl: vcoord/12k_top-64{m,i}.ascii) are not shipped: a namelist names the
user's own copy (tests/golden/vcoord holds the 64-level pair and an 80-level pair made by the same rule)."""
import os

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "vcoord")
P0 = 100000.0  # physical_constants.F90:26


class HvCoord:
    def __init__(self, vfile_mid=None, vfile_int=None, nlev=None):
        """nlev: the level count the caller is built for (the reference's plev); None: whatever the mid-level file holds.
        The interface file must then hold nlev + 1 levels (plevp)."""
        vfile_mid = vfile_mid or os.path.join(DATA, "acme-72m.ascii")
        vfile_int = vfile_int or os.path.join(DATA, "acme-72i.ascii")
        self.hyai, self.hybi = self._read(vfile_int)
        self.hyam, self.hybm = self._read(vfile_mid)
        plev = int(nlev) if nlev is not None else self.hyam.size
        # the reference's checks and messages (hybvcoord_mod.F90:76-102), first failure reported
        for name, arr, want, what in (("hyai", self.hyai, plev + 1, "plevp"), ("hybi", self.hybi, plev + 1, "plevp"),
                                      ("hyam", self.hyam, plev, "plev"), ("hybm", self.hybm, plev, "plev")):
            if arr.size != want:
                raise ValueError("Error: %s input file and HOMME %s do not match %d %d" % (name, what, want, arr.size))
        self.nlev, self.nlevp = plev, plev + 1
        self.ps0 = P0
        self.etam = self.hyam + self.hybm   # :170-171
        self.etai = self.hyai + self.hybi

    @staticmethod
    def _read(path):
        toks = []
        with open(path) as f:
            for line in f:
                line = line.split("!")[0].strip()
                if line:
                    toks += line.split()
        n = int(toks[0])
        a = np.array(toks[1:1 + n], dtype=np.float64)
        if int(toks[1 + n]) != n:
            raise ValueError("malformed vertical coordinate file " + path)
        b = np.array(toks[2 + n:2 + 2 * n], dtype=np.float64)
        return a, b
