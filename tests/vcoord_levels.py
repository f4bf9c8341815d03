"""The evenly-spaced-in-z hybrid grids of the reference's DCMIP 1-1 set-up (write_level_files, dcmip_wrapper_mod.F90:316-358), restated:
nlev + 1 interfaces evenly spaced in z from z_top = 12 000 m down to 0, eta = exp(-z/H) of the isothermal atmosphere (H = Rd*T0/g,
T0 = 300 K), B = ((eta - eta_top)/(1 - eta_top))^2, A = eta - B, mid-level coefficients the means of their interfaces.  The reference
ships the 64-level pair made this way (12k_top-64{m,i}.ascii, tests/golden/vcoord); the 80-level pair beside it is made by
`python tests/vcoord_levels.py 80` and pinned to this formula by tests/test_nlev80_cpu.py.  The files are written as the reference
writes them (list-directed output of a double: 17 significant digits), which is the format HvCoord reads."""
import os

import numpy as np

VC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcoord")
Z_TOP = 12000.0
RD, G, T0 = 287.04, 9.80616, 300.0   # physical_constants.F90 (Rgas, g); dcmip_wrapper_mod.F90:28
H = RD * T0 / G
DIGITS = 17                           # significant digits of a printed value


def levels(nlev):
    """-> hyai, hybi [nlev + 1], hyam, hybm [nlev]"""
    k = np.arange(nlev + 1, dtype=np.float64)
    zi = Z_TOP - Z_TOP * k / nlev
    eta = np.exp(-zi / H)
    r = (eta - eta[0]) / (1.0 - eta[0])
    bi = r * r
    ai = eta - bi
    return ai, bi, 0.5 * (ai[1:] + ai[:-1]), 0.5 * (bi[1:] + bi[:-1])


def fmt(x):
    """a double as list-directed Fortran output prints it: 17 significant digits, plain in [0.1, 10) and for 0, else d.dddE+xxx"""
    x = float(x)
    if x == 0.0:
        return "   0.0000000000000000     "
    m, e = ("%.*E" % (DIGITS - 1, x)).split("E")
    e = int(e)
    if e == -1:
        return "  %.*f     " % (DIGITS, x)
    if e == 0:
        return "   %.*f     " % (DIGITS - 1, x)
    return "   %sE%+04d" % (m, e)


def render(a, b, names):
    n = len(a)
    out = ["%12d  ! %s" % (n, names[0])] + [fmt(x) for x in a] + ["%12d  ! %s" % (n, names[1])] + [fmt(x) for x in b]
    return "\n".join(out) + "\n"


def files(nlev):
    """-> {file name: text} of the mid-level and the interface file"""
    ai, bi, am, bm = levels(nlev)
    return {"12k_top-%dm.ascii" % nlev: render(am, bm, ("hyam", "hybm")), "12k_top-%di.ascii" % nlev: render(ai, bi, ("hyai", "hybi"))}


def paths(nlev):
    return os.path.join(VC, "12k_top-%dm.ascii" % nlev), os.path.join(VC, "12k_top-%di.ascii" % nlev)


def ulp_last_digit(x):
    """one unit in the last printed digit of x (0 prints as 0: no digits to compare)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x > 0, 10.0 ** (np.floor(np.log10(np.where(x > 0, x, 1.0))) - (DIGITS - 1)), 0.0)


if __name__ == "__main__":
    import sys
    for name, text in files(int(sys.argv[1])).items():
        with open(os.path.join(VC, name), "w") as f:
            f.write(text)
