"""Float64 definitions of the lighting and sampling helpers, and the seeded generators of well-conditioned inputs for them.

Shared by test_oracle_independent.py (the oracle's single-call hooks against these models) and test_helper_probe_host.py (the
oracle's probe rows against the same models, on the rows the GPU probe test also runs). Each model is written from its
mathematical definition (microfacet BRDF, Heitz' visible-normal sampling) in vectorised numpy, in a different shape than the
shader's statement order. Reference text: shaders/rt_utils.slang:150-274."""
import numpy as np

PI_REF = 3.14159        # the literal most helpers use (rt_utils.slang:172,223,230,260)
PI_VNDF = 3.14159265    # sample_ggx_vndf's (rt_utils.slang:192)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def onb(n):
    """Duff et al. 2017 branchless orthonormal basis, the construction build_onb names (rt_utils.slang:150-156)."""
    s = np.where(n[..., 2] >= 0.0, 1.0, -1.0)
    a = -1.0 / (s + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    t = np.stack([1.0 + s * n[..., 0] ** 2 * a, s * b, -s * n[..., 0]], -1)
    bt = np.stack([b, s + n[..., 1] ** 2 * a, -n[..., 1]], -1)
    return t, bt


def brdf_light(P, N, V, albedo, rough, metal, Le, X, Nl):
    """Unshadowed radiance from a light sample X (normal Nl, emission Le) towards the viewer: GGX specular with the
    height-correlated Smith visibility + Lambert diffuse weighted by (1 - metallic)(1 - F), times cos cos / d^2."""
    d = X - P
    dist = np.maximum(np.linalg.norm(d, axis=-1), 1e-4)
    Ld = d / dist[:, None]
    cos_s = np.einsum("ij,ij->i", N, Ld)
    cos_l = -np.einsum("ij,ij->i", Nl, Ld)
    lit = (cos_s > 0) & (cos_l > 0)
    H = unit(V + Ld)
    nh = np.maximum(np.einsum("ij,ij->i", N, H), 0.0)
    vh = np.maximum(np.einsum("ij,ij->i", V, H), 0.0)
    nv = np.maximum(np.einsum("ij,ij->i", N, V), 1e-3)
    alpha = rough ** 2
    D = alpha ** 2 / (PI_REF * ((nh ** 2) * (alpha ** 2 - 1.0) + 1.0) ** 2)
    F0 = 0.04 + (albedo - 0.04) * metal[:, None]
    Fr = F0 + (1.0 - F0) * ((1.0 - vh) ** 5)[:, None]
    lam_v = cos_s * np.sqrt(nv ** 2 * (1 - alpha ** 2) + alpha ** 2)
    lam_l = nv * np.sqrt(cos_s ** 2 * (1 - alpha ** 2) + alpha ** 2)
    Vis = 0.5 / np.maximum(lam_v + lam_l, 1e-4)
    spec = (D * Vis)[:, None] * Fr
    diff = albedo * (1.0 - metal)[:, None] * (1.0 - Fr) / PI_REF
    G = cos_s * cos_l / np.maximum(dist ** 2, 1e-4)
    out = Le * (diff + spec) * G[:, None]
    out[~lit] = 0.0
    return out


def vndf_sample(N, V, rough, u1, u2):
    """Heitz 2018, "Sampling the GGX Distribution of Visible Normals", in the tangent frame of N: stretch the view
    vector, sample the projected disk (re-parameterised by the visible half), project onto the hemisphere, unstretch."""
    T, B = onb(N)
    Vl = np.stack([np.einsum("ij,ij->i", V, T), np.einsum("ij,ij->i", V, B), np.einsum("ij,ij->i", V, N)], -1)
    a = np.maximum(rough ** 2, 1e-3)[:, None]
    Vh = unit(Vl * np.concatenate([a, a, np.ones_like(a)], 1))
    lensq = Vh[:, 0] ** 2 + Vh[:, 1] ** 2
    T1 = np.where((lensq > 0)[:, None], np.stack([-Vh[:, 1], Vh[:, 0], np.zeros_like(lensq)], -1) / np.sqrt(np.where(lensq > 0, lensq, 1.0))[:, None],
                  np.array([1.0, 0.0, 0.0]))
    T2 = np.cross(Vh, T1)
    r = np.sqrt(u1); phi = 2.0 * PI_VNDF * u2
    t1 = r * np.cos(phi); t2 = r * np.sin(phi)
    s = 0.5 * (1.0 + Vh[:, 2])
    t2 = (1.0 - s) * np.sqrt(1.0 - t1 ** 2) + s * t2
    Nh = t1[:, None] * T1 + t2[:, None] * T2 + np.sqrt(np.maximum(0.0, 1.0 - t1 ** 2 - t2 ** 2))[:, None] * Vh
    Hl = unit(np.stack([a[:, 0] * Nh[:, 0], a[:, 0] * Nh[:, 1], np.maximum(0.0, Nh[:, 2])], -1))
    return T * Hl[:, 0:1] + B * Hl[:, 1:2] + N * Hl[:, 2:3]


def gi_pdf(P, N, albedo, metal, X, rad):
    """Target function of a GI sample: the largest channel of radiance x Lambert BRDF x cosine at the shaded point."""
    w = X - P
    cosv = np.maximum(np.einsum("ij,ij->i", N, w / np.maximum(np.linalg.norm(w, axis=1), 1e-4)[:, None]), 0.0)
    return (rad * albedo * ((1.0 - metal) / PI_REF * cosv)[:, None]).max(axis=1), cosv


# ---- seeded, well-conditioned inputs (float64; the callers round them to fp32) ---------------------------------------------
def light_inputs(rng, n):
    """(P, N, V, albedo, rough, metal, Le, X, Nl): a viewer above the surface, a light 0.2 to 6 away in the upper hemisphere."""
    P = rng.uniform(-2, 2, (n, 3)); N = unit(rng.normal(size=(n, 3))); V = unit(N + 0.9 * unit(rng.normal(size=(n, 3))))
    X = P + unit(N + 0.8 * unit(rng.normal(size=(n, 3)))) * rng.uniform(0.2, 6.0, (n, 1))
    Nl = unit(P - X + 0.7 * rng.normal(size=(n, 3)))
    albedo = rng.uniform(0.05, 0.95, (n, 3)); rough = rng.uniform(0.05, 1.0, n); metal = rng.uniform(0, 1, n) * (rng.random(n) > 0.5)
    Le = rng.uniform(0.5, 12.0, (n, 3))
    return P, N, V, albedo, rough, metal, Le, X, Nl


def vndf_inputs(rng, n):
    """(N, V, rough, u1, u2): a viewer above the surface, roughness from 0.02."""
    N = unit(rng.normal(size=(n, 3))); V = unit(N + 0.95 * unit(rng.normal(size=(n, 3))))
    rough = rng.uniform(0.02, 1.0, n); u1 = rng.random(n); u2 = rng.random(n)
    return N, V, rough, u1, u2


def gi_inputs(rng, n):
    """(P, N, albedo, metal, X, rad)."""
    P = rng.uniform(-3, 3, (n, 3)); N = unit(rng.normal(size=(n, 3))); X = P + rng.normal(size=(n, 3)) * 2.0
    albedo = rng.uniform(0, 1, (n, 3)); metal = rng.uniform(0, 1, n); rad = rng.uniform(0, 5, (n, 3))
    return P, N, albedo, metal, X, rad
