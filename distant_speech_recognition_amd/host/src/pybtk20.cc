// pybtk20.cc -- Python binding of the C++ node layer (libbtk20hip.so): the classes the reference exposes through SWIG
// (stream/stream.i, feature/feature.i, modulated/modulated.i, beamformer/beamformer.i, postfilter/postfilter.i,
// dereverberation/dereverberation.i, convolution/convolution.i, sad/sad.i, objective_measure/objective_measure.i,
// localization/localization.i:128-260) bound with pybind11 under the same names.
//   * a bound object IS the C++ node: the holder shares Countable's intrusive count with the refcountable_ptrs the nodes keep
//     of each other, so Python and C++ references are one population;
//   * next() returns a numpy VIEW of the node's vector_ (no copy; the array keeps the node alive) -- the reference's typemap
//     does the same (include/vector.i:290-305);
//   * jiterator_error surfaces as StopIteration, the rest of the j_error family as Python exceptions of the same names;
//   * PyVectorFloatFeatureStream / PyVectorComplexFeatureStream wrap any Python object with size() / __iter__ / next() /
//     reset() as a C++ source node (reference stream/pyStream.h:25-168), so Python code can feed C++ nodes.
#include <pybind11/complex.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <complex>
#include <vector>

#include "beamformer/beamformer.h"
#include "dereverberation/dereverberation.h"
#include "aec/aec.h"
#include "convolution/convolution.h"
#include "feature/feature.h"
#include "modulated/modulated.h"
#include "postfilter/postfilter.h"
#include "postfilter/spectralsubtraction.h"
#include "postfilter/binauralprocessing.h"
#include "sad/sad.h"
#include "objective_measure/objective_measure.h"
#include "localization/localization.h"

namespace py = pybind11;
typedef std::complex<double> cd;

// intrusive holder: one reference count per object, kept in Countable
template <class T>
class cref {
 public:
  cref(T* p = nullptr) : p_(p) { if (p_) p_->increment(); }
  cref(const cref& o) : p_(o.p_) { if (p_) p_->increment(); }
  cref& operator=(const cref& o) { if (p_ != o.p_) { release(); p_ = o.p_; if (p_) p_->increment(); } return *this; }
  ~cref() { release(); }
  T* get() const { return p_; }
 private:
  void release() { if (!p_) return; if (p_->unique()) delete p_; else p_->decrement(); p_ = nullptr; }
  T* p_;
};
PYBIND11_DECLARE_HOLDER_TYPE(T, cref<T>, true);

namespace {

// ---- numpy <-> gsl PODs
struct GslVec {
  gsl_vector* v;
  explicit GslVec(const py::array_t<double, py::array::c_style | py::array::forcecast>& a) : v(gsl_vector_calloc((size_t)a.size())) {
    memcpy(v->data, a.data(), sizeof(double) * (size_t)a.size());
  }
  ~GslVec() { gsl_vector_free(v); }
  GslVec(const GslVec&) = delete;
};
struct GslMat {
  gsl_matrix* m;
  explicit GslMat(const py::array_t<double, py::array::c_style | py::array::forcecast>& a) {
    if (a.ndim() != 2) throw jdimension_error("expected a 2-d array, got %d-d", (int)a.ndim());
    m = gsl_matrix_alloc((size_t)a.shape(0), (size_t)a.shape(1));
    memcpy(m->data, a.data(), sizeof(double) * (size_t)a.size());
  }
  ~GslMat() { gsl_matrix_free(m); }
  GslMat(const GslMat&) = delete;
};
struct GslCVec {
  gsl_vector_complex* v;
  explicit GslCVec(const py::array_t<cd, py::array::c_style | py::array::forcecast>& a) : v(gsl_vector_complex_calloc((size_t)a.size())) {
    memcpy(v->data, a.data(), sizeof(double) * 2 * (size_t)a.size());
  }
  ~GslCVec() { gsl_vector_complex_free(v); }
  GslCVec(const GslCVec&) = delete;
};
struct GslCMat {
  gsl_matrix_complex* m;
  explicit GslCMat(const py::array_t<cd, py::array::c_style | py::array::forcecast>& a) {
    if (a.ndim() != 2) throw jdimension_error("expected a 2-d array, got %d-d", (int)a.ndim());
    m = gsl_matrix_complex_alloc((size_t)a.shape(0), (size_t)a.shape(1));
    memcpy(m->data, a.data(), sizeof(double) * 2 * (size_t)a.size());
  }
  ~GslCMat() { gsl_matrix_complex_free(m); }
  GslCMat(const GslCMat&) = delete;
};

// views of node-owned storage (kept alive by `owner`), copies of transient views
py::array view(const gsl_vector_float* v, py::handle owner) { return py::array_t<float>({(py::ssize_t)v->size}, {(py::ssize_t)sizeof(float)}, v->data, owner); }
py::array view(const gsl_vector* v, py::handle owner) { return py::array_t<double>({(py::ssize_t)v->size}, {(py::ssize_t)sizeof(double)}, v->data, owner); }
py::array view(const gsl_vector_complex* v, py::handle owner) { return py::array_t<cd>({(py::ssize_t)v->size}, {(py::ssize_t)sizeof(cd)}, reinterpret_cast<const cd*>(v->data), owner); }
py::array copy_of(const gsl_vector_complex* v) {
  py::array_t<cd> a((py::ssize_t)v->size);
  memcpy(static_cast<void*>(a.mutable_data()), v->data, sizeof(cd) * v->size);
  return std::move(a);
}
py::array copy_of(const gsl_matrix_complex* m) {
  py::array_t<cd> a({(py::ssize_t)m->size1, (py::ssize_t)m->size2});
  for (size_t i = 0; i < m->size1; i++) memcpy(static_cast<void*>(a.mutable_data(i, 0)), m->data + 2 * i * m->tda, sizeof(cd) * m->size2);
  return std::move(a);
}

// ---- a Python object as a source node (reference stream/pyStream.h:25-168)
template <class Base, class VecT, class T>
class PyStream : public Base, public BlockSource {
 public:
  PyStream(py::object c, const String& nm) : Base(size_of_(c), nm), cont_(c), iter_(c.attr("__iter__")()) {}
  ~PyStream() { py::gil_scoped_acquire g; cont_ = py::object(); iter_ = py::object(); }
  const VecT* next(int frame_no = -5) override {
    if (frame_no == this->frame_no_) return this->vector_;
    py::gil_scoped_acquire g;
    py::object o;
    try {
      o = py::hasattr(iter_, "next") ? iter_.attr("next")() : iter_.attr("__next__")();
    } catch (py::error_already_set& e) {
      if (e.matches(PyExc_StopIteration)) { this->is_end_ = true; throw jiterator_error("No more samples!"); }
      throw;
    }
    py::array_t<T, py::array::c_style | py::array::forcecast> a(o);
    if ((size_t)a.size() < this->size_) throw jdimension_error("Python source returned %d items, the stream has %d", (int)a.size(), (int)this->size_);
    memcpy(this->vector_->data, a.data(), sizeof(T) * this->size_);
    this->increment_();
    return this->vector_;
  }
  void reset() override {
    py::gil_scoped_acquire g;
    cont_.attr("reset")();
    iter_ = cont_.attr("__iter__")();
    Base::reset();
  }
  py::object python_object() const { return cont_; }
  // BlockSource: a GPU-backed Python beamformer (pybeamformer.*, or anything with device_block() -> complex [.. K][T], optionally
  // _output_version() / _advance_to(idx)) hands its whole block to a batching C++ consumer; plain iterators have none and are drained
  bool has_block() override { py::gil_scoped_acquire g; return py::hasattr(cont_, "device_block"); }
  unsigned long block_version() override {
    py::gil_scoped_acquire g;
    return py::hasattr(cont_, "_output_version") ? cont_.attr("_output_version")().template cast<unsigned long>() : 0ul;
  }
  const std::vector<float>& block(long& Tn) override {
    py::gil_scoped_acquire g;
    py::object b = cont_.attr("device_block")();
    if (py::hasattr(b, "detach")) b = b.attr("detach")().attr("cpu")().attr("numpy")();      // a torch tensor
    py::array_t<std::complex<float>, py::array::c_style | py::array::forcecast> a(b);
    if (a.ndim() < 2) throw jdimension_error("device_block() must return [.. K][T], got %d-d", (int)a.ndim());
    const size_t K = (size_t)a.shape(a.ndim() - 2);
    Tn = (long)a.shape(a.ndim() - 1);
    blk_.resize(2 * K * (size_t)Tn);
    memcpy(blk_.data(), a.data(), sizeof(float) * blk_.size());
    return blk_;
  }
  void advance_to(long idx) override {
    py::gil_scoped_acquire g;
    if (py::hasattr(cont_, "_advance_to")) cont_.attr("_advance_to")(idx);
  }
  // blocks of a bounded number of frames (modulated/modulated.h): _block_base() = stream index of the block's first frame,
  // _next_block() moves the object on to its following block and returns False at the end of the stream
  long block_base() override {
    py::gil_scoped_acquire g;
    return py::hasattr(cont_, "_block_base") ? cont_.attr("_block_base")().template cast<long>() : 0l;
  }
  bool next_block() override {
    py::gil_scoped_acquire g;
    return py::hasattr(cont_, "_next_block") ? cont_.attr("_next_block")().template cast<bool>() : false;
  }
 private:
  static unsigned size_of_(const py::object& c) { return c.attr("size")().cast<unsigned>(); }
  py::object cont_, iter_;
  std::vector<float> blk_;
};
typedef PyStream<VectorFloatFeatureStream, gsl_vector_float, float> PyVectorFloatFeatureStream;
typedef PyStream<VectorComplexFeatureStream, gsl_vector_complex, cd> PyVectorComplexFeatureStream;
typedef PyStream<VectorFeatureStream, gsl_vector, double> PyVectorFeatureStream;

// the methods of DOAEstimatorSRPBase (beamformer.i:677-708) on a bound class T that derives from it.  nbest_rps / nbest_doas /
// response_power_matrix are numpy VIEWS of the estimator's own storage (kept alive by the array), like next()'s vector.
template <class T, class Cls>
void def_srp_base(Cls& cls)
{
  auto vec = [](py::object self) { const gsl_vector* v = self.cast<T&>().nbest_rps();
    return py::array(py::array_t<double>({(py::ssize_t)v->size}, {(py::ssize_t)sizeof(double)}, v->data, self)); };
  auto doa = [](py::object self) { const gsl_matrix* a = self.cast<T&>().nbest_doas();
    return py::array(py::array_t<double>({(py::ssize_t)a->size1, (py::ssize_t)a->size2}, {(py::ssize_t)(sizeof(double) * a->tda), (py::ssize_t)sizeof(double)}, a->data, self)); };
  auto mat = [](py::object self) { const gsl_matrix* a = self.cast<T&>().response_power_matrix();
    return py::array(py::array_t<double>({(py::ssize_t)a->size1, (py::ssize_t)a->size2}, {(py::ssize_t)(sizeof(double) * a->tda), (py::ssize_t)sizeof(double)}, a->data, self)); };
  auto search = [](T& e, float minTheta, float maxTheta, float minPhi, float maxPhi, float widthTheta, float widthPhi) {
    e.set_search_param(minTheta, maxTheta, minPhi, maxPhi, widthTheta, widthPhi); };
  cls.def("nbest_rps", vec).def("getNBestRPs", vec)
      .def("nbest_doas", doa).def("getNBestDOAs", doa)
      .def("response_power_matrix", mat).def("getResponsePowerMatrix", mat)
      .def("energy", [](T& e) { return e.energy(); }).def("getEnergy", [](T& e) { return e.energy(); })
      .def("final_nbest_hypotheses", [](T& e) { e.final_nbest_hypotheses(); })
      .def("getFinalNBestHypotheses", [](T& e) { e.final_nbest_hypotheses(); })
      .def("set_energy_threshold", [](T& e, float th) { e.set_energy_threshold(th); }, py::arg("engeryThreshold"))
      .def("setEnergyThreshold", [](T& e, float th) { e.set_energy_threshold(th); }, py::arg("engeryThreshold"))
      .def("set_frequency_range", [](T& e, unsigned lo, unsigned hi) { e.set_frequency_range(lo, hi); }, py::arg("fbinMin"), py::arg("fbinMax"))
      .def("setFrequencyRange", [](T& e, unsigned lo, unsigned hi) { e.set_frequency_range(lo, hi); }, py::arg("fbinMin"), py::arg("fbinMax"))
      .def("init_accs", [](T& e) { e.init_accs(); }).def("initAccs", [](T& e) { e.init_accs(); })
      .def("set_search_param", search, py::arg("minTheta") = (float)(-M_PI / 2), py::arg("maxTheta") = (float)(M_PI / 2),
           py::arg("minPhi") = (float)(-M_PI / 2), py::arg("maxPhi") = (float)(M_PI / 2), py::arg("widthTheta") = 0.1f, py::arg("widthPhi") = 0.1f)
      .def("setSearchParam", search, py::arg("minTheta") = (float)(-M_PI / 2), py::arg("maxTheta") = (float)(M_PI / 2),
           py::arg("minPhi") = (float)(-M_PI / 2), py::arg("maxPhi") = (float)(M_PI / 2), py::arg("widthTheta") = 0.1f, py::arg("widthPhi") = 0.1f)
      // the grid and the accumulated powers as they stand after the frame served last (copies)
      .def("search_thetas", [](T& e) { const std::vector<double>& v = e.search_thetas(); return py::array_t<double>((py::ssize_t)v.size(), v.data()); })
      .def("accumulated_rps", [](T& e) { const std::vector<double>& v = e.accumulated_rps(); return py::array_t<double>((py::ssize_t)v.size(), v.data()); });
}

// a bound node is used as it is; any other Python object with size() / __iter__ / next() / reset() becomes a source node (the
// reference wants the explicit PyVector*FeatureStreamPtr(obj) wrapper, stream/pyStream.h:25-168; both spellings work here)
VectorComplexFeatureStreamPtr as_cstream(const py::object& o)
{
  if (py::isinstance<VectorComplexFeatureStream>(o)) return VectorComplexFeatureStreamPtr(o.cast<VectorComplexFeatureStream*>());
  return VectorComplexFeatureStreamPtr(new PyVectorComplexFeatureStream(o, "PyVectorComplexFeatureStream"));
}
VectorFloatFeatureStreamPtr as_fstream(const py::object& o)
{
  if (py::isinstance<VectorFloatFeatureStream>(o)) return VectorFloatFeatureStreamPtr(o.cast<VectorFloatFeatureStream*>());
  return VectorFloatFeatureStreamPtr(new PyVectorFloatFeatureStream(o, "PyVectorFloatFeatureStream"));
}
VectorFeatureStreamPtr as_dstream(const py::object& o)
{
  if (py::isinstance<VectorFeatureStream>(o)) return VectorFeatureStreamPtr(o.cast<VectorFeatureStream*>());
  return VectorFeatureStreamPtr(new PyVectorFeatureStream(o, "PyVectorFeatureStream"));
}
py::array dense_of(gsl_matrix* m)
{
  py::array_t<double> a({(py::ssize_t)m->size1, (py::ssize_t)m->size2});
  for (size_t i = 0; i < m->size1; i++) memcpy(a.mutable_data(i, 0), m->data + i * m->tda, sizeof(double) * m->size2);
  return std::move(a);
}
// matrix(matrix): the reference fills the caller's matrix; here the dense matrix is returned, and copied into `out` where one is given
template <class T>
py::array matrix_of(T& node, size_t rows, size_t cols, py::object out)
{
  gsl_matrix* m = gsl_matrix_alloc(rows, cols);
  try { node.matrix(m); } catch (...) { gsl_matrix_free(m); throw; }
  py::array a = dense_of(m);
  gsl_matrix_free(m);
  if (!out.is_none()) out.attr("__setitem__")(py::ellipsis(), a);
  return a;
}
py::array block_of(BlockSource& b)
{
  long T = 0;
  const std::vector<float>& y = b.block(T);
  const py::ssize_t K = T > 0 ? (py::ssize_t)(y.size() / 2 / (size_t)T) : 0;
  py::array_t<std::complex<float>> a({(py::ssize_t)1, K, (py::ssize_t)T});
  if (T > 0) memcpy(static_cast<void*>(a.mutable_data()), y.data(), sizeof(float) * 2 * (size_t)K * (size_t)T);
  return std::move(a);
}

template <class S, class C>
void bind_stream_methods(C& cls)
{
  cls.def("next", [](py::object self, int frame_no) { S& s = self.cast<S&>(); return view(s.next(frame_no), self); }, py::arg("frame_no") = -5)
      .def("__next__", [](py::object self) { S& s = self.cast<S&>(); return view(s.next(-5), self); })
      .def("__iter__", [](py::object self) { self.attr("reset")(); return self; })
      .def("current", [](py::object self) { S& s = self.cast<S&>(); return view(s.current(), self); })
      .def("reset", [](S& s) { s.reset(); })
      .def("size", &S::size)
      .def("is_end", [](S& s) { return s.is_end(); })
      .def("frame_no", [](S& s) { return s.frame_no(); })
      .def("name", [](S& s) { return std::string(s.name()); });
}

}  // namespace

PYBIND11_MODULE(_btk20cpp, m)
{
  m.doc() = "C++ node layer of the MI355X subband-beamforming engine (libbtk20hip.so) under the reference's class names";

  // ---- exceptions: jiterator_error ends an iteration, the rest keep their names
  static py::exception<j_error> ex_j(m, "j_error");
  static py::exception<j_error> ex_alloc(m, "jallocation_error", ex_j.ptr());
  static py::exception<j_error> ex_cons(m, "jconsistency_error", ex_j.ptr());
  static py::exception<j_error> ex_dim(m, "jdimension_error", ex_j.ptr());
  static py::exception<j_error> ex_idx(m, "jindex_error", ex_j.ptr());
  static py::exception<j_error> ex_io(m, "jio_error", ex_j.ptr());
  static py::exception<j_error> ex_par(m, "jparameter_error", ex_j.ptr());
  static py::exception<j_error> ex_num(m, "jnumeric_error", ex_j.ptr());
  py::register_exception_translator([](std::exception_ptr p) {
    try {
      if (p) std::rethrow_exception(p);
    } catch (j_error& e) {
      switch (e.getCode()) {
        case JITERATOR: PyErr_SetString(PyExc_StopIteration, e.what()); break;
        case JALLOCATION: py::set_error(ex_alloc, e.what()); break;
        case JCONSISTENCY: py::set_error(ex_cons, e.what()); break;
        case JDIMENSION: py::set_error(ex_dim, e.what()); break;
        case JINDEX: py::set_error(ex_idx, e.what()); break;
        case JIO: py::set_error(ex_io, e.what()); break;
        case JPARAMETER: py::set_error(ex_par, e.what()); break;
        case JNUMERIC: py::set_error(ex_num, e.what()); break;
        default: py::set_error(ex_j, e.what());
      }
    }
  });

  // ---- stream bases
  py::class_<VectorFloatFeatureStream, cref<VectorFloatFeatureStream>> vf(m, "VectorFloatFeatureStream");
  bind_stream_methods<VectorFloatFeatureStream>(vf);
  py::class_<VectorFeatureStream, cref<VectorFeatureStream>> vd(m, "VectorFeatureStream");
  bind_stream_methods<VectorFeatureStream>(vd);
  py::class_<VectorComplexFeatureStream, cref<VectorComplexFeatureStream>> vc(m, "VectorComplexFeatureStream");
  bind_stream_methods<VectorComplexFeatureStream>(vc);

  py::class_<PyVectorFloatFeatureStream, VectorFloatFeatureStream, cref<PyVectorFloatFeatureStream>>(m, "PyVectorFloatFeatureStreamPtr")
      .def(py::init([](py::object c, const std::string& nm) { return new PyVectorFloatFeatureStream(c, nm); }), py::arg("c"), py::arg("nm") = "PyVectorFloatFeatureStream")
      .def("python_object", &PyVectorFloatFeatureStream::python_object);
  py::class_<PyVectorComplexFeatureStream, VectorComplexFeatureStream, cref<PyVectorComplexFeatureStream>>(m, "PyVectorComplexFeatureStreamPtr")
      .def(py::init([](py::object c, const std::string& nm) { return new PyVectorComplexFeatureStream(c, nm); }), py::arg("c"), py::arg("nm") = "PyVectorComplexFeatureStream")
      .def("python_object", &PyVectorComplexFeatureStream::python_object);

  // ---- feature/feature.h
  py::class_<SampleFeature, VectorFloatFeatureStream, cref<SampleFeature>>(m, "SampleFeaturePtr")
      .def(py::init([](const std::string& fn, unsigned block_len, unsigned shift_len, bool pad_zeros, const std::string& nm) {
             return new SampleFeature(fn, block_len, shift_len, pad_zeros, nm);
           }), py::arg("fn") = "", py::arg("block_len") = 320, py::arg("shift_len") = 160, py::arg("pad_zeros") = false, py::arg("nm") = "Sample")
      .def("read", [](SampleFeature& s, const std::string& fn, int format, int samplerate, int chX, int chN, int cfrom, int to, int outsamplerate, float norm) {
             return s.read(fn, format, samplerate, chX, chN, cfrom, to, outsamplerate, norm);
           }, py::arg("fn"), py::arg("format") = 0, py::arg("samplerate") = 16000, py::arg("chX") = 1, py::arg("chN") = 1, py::arg("cfrom") = 0,
           py::arg("to") = -1, py::arg("outsamplerate") = -1, py::arg("norm") = 0.0f)
      .def("set_samples", [](SampleFeature& s, py::array_t<float, py::array::c_style | py::array::forcecast> a) { s.set_samples(a.data(), (size_t)a.size()); })
      .def("holds_pcm16", [](SampleFeature& s) { return s.pcm16() != NULL; })   // every loaded sample is an integer of the int16 range
      .def("samplerate", &SampleFeature::getSampleRate)
      .def("getSampleRate", &SampleFeature::getSampleRate)
      .def("getChanN", &SampleFeature::getChanN)
      .def("samplesN", &SampleFeature::samplesN)
      .def("write", [](SampleFeature& s, const std::string& fn, int format, int sampleRate) { s.write(fn, format, sampleRate); },
           py::arg("fn"), py::arg("format") = (int)(sndfile::SF_FORMAT_WAV | sndfile::SF_FORMAT_PCM_16), py::arg("sampleRate") = -1)
      .def("cut", &SampleFeature::cut, py::arg("cfrom"), py::arg("cto"))
      .def("randomize", &SampleFeature::randomize, py::arg("startX"), py::arg("endX"), py::arg("sigma2"))
      .def("exit", &SampleFeature::exit)
      .def("data", [](SampleFeature& s) {
             const gsl_vector_float* v = s.data();
             py::array_t<float> a((py::ssize_t)v->size);
             if (v->size) memcpy(a.mutable_data(), v->data, sizeof(float) * v->size);
             return a; })
      .def("dataDouble", [](SampleFeature& s) {
             const gsl_vector* v = s.dataDouble();
             py::array_t<double> a((py::ssize_t)v->size);
             if (v->size) memcpy(a.mutable_data(), v->data, sizeof(double) * v->size);
             return a; })
      .def("copySamples", [](SampleFeature& s, SampleFeature* src, unsigned cfrom, unsigned to) { SampleFeaturePtr p(src); s.copySamples(p, cfrom, to); },
           py::arg("src"), py::arg("cfrom"), py::arg("to"))
      .def("zeroMean", &SampleFeature::zeroMean)
      .def("addWhiteNoise", &SampleFeature::addWhiteNoise, py::arg("snr"))
      .def("setSamples", [](SampleFeature& s, py::array_t<double, py::array::c_style | py::array::forcecast> a, unsigned sampleRate) {
             GslVec v(a); s.setSamples(v.v, sampleRate); }, py::arg("samples"), py::arg("sampleRate"));
  // the TDOA front end (feature/feature.i:525-531, 567-573)
  py::class_<HammingFeature, VectorFloatFeatureStream, cref<HammingFeature>>(m, "HammingFeaturePtr")
      .def(py::init([](py::object samp, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             return new HammingFeature(sp, nm);
           }), py::arg("samp"), py::arg("nm") = "Hamming");
  py::class_<FFTFeature, VectorComplexFeatureStream, cref<FFTFeature>>(m, "FFTFeaturePtr")
      .def(py::init([](py::object samp, unsigned fft_len, const std::string& nm, long block_frames) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             return new FFTFeature(sp, fft_len, nm, block_frames);
           }), py::arg("samp"), py::arg("fft_len") = 512, py::arg("nm") = "FFT", py::arg("block_frames") = 0)
      .def("fftLen", &FFTFeature::fftLen)
      .def("windowLen", &FFTFeature::windowLen)
      .def("nBlocks", &FFTFeature::nBlocks)
      .def("subsamplerate", &FFTFeature::subsamplerate)
      .def("subSampRate", &FFTFeature::subSampRate)
      .def("set_block_frames", &FFTFeature::set_block_frames, py::arg("n"))
      .def("block_frames", &FFTFeature::block_frames)
      .def("launches", &FFTFeature::launches)
      .def("has_sample_chain", &FFTFeature::has_sample_chain)
      // up to nmax un-windowed sample blocks of the chain as float32 [n][windowLen] (a copy), every node of the chain advanced by n
      .def("pull_sample_blocks", [](FFTFeature& f, long nmax) {
             if (nmax < 0) nmax = 0;
             std::vector<float> buf((size_t)nmax * f.windowLen());
             const long n = f.pull_sample_blocks(buf.data(), nmax);
             py::array_t<float> a({(py::ssize_t)n, (py::ssize_t)f.windowLen()});
             if (n > 0) memcpy(a.mutable_data(), buf.data(), sizeof(float) * (size_t)n * f.windowLen());
             return a; }, py::arg("nmax"));

  // the recogniser's front end (feature/feature.i: PreemphasisFeature, SpectralPowerFeature, VTLNFeature, MelFeature, LogFeature,
  // CepstralFeature, StorageFeature); block_frames / set_block_frames / launches are the engine's additions
  py::class_<PyVectorFeatureStream, VectorFeatureStream, cref<PyVectorFeatureStream>>(m, "PyVectorFeatureStreamPtr")
      .def(py::init([](py::object c, const std::string& nm) { return new PyVectorFeatureStream(c, nm); }), py::arg("c"), py::arg("nm") = "PyVectorFeatureStream")
      .def("python_object", &PyVectorFeatureStream::python_object);
  py::class_<PreemphasisFeature, VectorFloatFeatureStream, cref<PreemphasisFeature>>(m, "PreemphasisFeaturePtr")
      .def(py::init([](py::object samp, double mu, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             return new PreemphasisFeature(sp, mu, nm);
           }), py::arg("samp"), py::arg("mu") = 0.95, py::arg("nm") = "Preemphasis")
      .def("next_speaker", &PreemphasisFeature::next_speaker)
      .def("nextSpeaker", &PreemphasisFeature::next_speaker);
  py::class_<StorageFeature, VectorFloatFeatureStream, cref<StorageFeature>>(m, "StorageFeaturePtr")
      .def(py::init([](py::object src, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(src);
             return new StorageFeature(sp, nm);
           }), py::arg("src"), py::arg("nm") = "Storage")
      .def("write", [](StorageFeature& s, const std::string& fn, bool plainText) { s.write(fn, plainText); }, py::arg("fileName"), py::arg("plainText") = false)
      .def("read", [](StorageFeature& s, const std::string& fn) { s.read(fn); }, py::arg("fileName"))
      .def("evaluate", &StorageFeature::evaluate);
  py::class_<SpectralPowerFeature, VectorFeatureStream, cref<SpectralPowerFeature>>(m, "SpectralPowerFeaturePtr")
      .def(py::init([](py::object fft, unsigned pow_num, const std::string& nm) {
             VectorComplexFeatureStreamPtr sp = as_cstream(fft);
             return new SpectralPowerFeature(sp, pow_num, nm);
           }), py::arg("fft"), py::arg("pow_num") = 0, py::arg("nm") = "Power")
      .def("set_block_frames", [](SpectralPowerFeature& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](SpectralPowerFeature& f) { return f.block_frames(); })
      .def("launches", [](SpectralPowerFeature& f) { return f.launches(); });
  py::class_<SpectralPowerFloatFeature, VectorFloatFeatureStream, cref<SpectralPowerFloatFeature>>(m, "SpectralPowerFloatFeaturePtr")
      .def(py::init([](py::object fft, unsigned powN, const std::string& nm) {
             VectorComplexFeatureStreamPtr sp = as_cstream(fft);
             return new SpectralPowerFloatFeature(sp, powN, nm);
           }), py::arg("fft"), py::arg("powN") = 0, py::arg("nm") = "Power");
  py::class_<VTLNFeature, VectorFeatureStream, cref<VTLNFeature>>(m, "VTLNFeaturePtr")
      .def(py::init([](py::object pow, unsigned coeff_num, double ratio, double edge, int version, const std::string& nm) {
             VectorFeatureStreamPtr sp = as_dstream(pow);
             return new VTLNFeature(sp, coeff_num, ratio, edge, version, nm);
           }), py::arg("pow"), py::arg("coeff_num") = 0, py::arg("ratio") = 1.0, py::arg("edge") = 1.0, py::arg("version") = 1, py::arg("nm") = "VTLN")
      .def("warp", &VTLNFeature::warp, py::arg("w"))
      .def("matrix", [](VTLNFeature& f, py::object out) { return matrix_of(f, f.size(), f.source_size(), out); }, py::arg("matrix") = py::none())
      .def("set_block_frames", [](VTLNFeature& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](VTLNFeature& f) { return f.block_frames(); })
      .def("launches", [](VTLNFeature& f) { return f.launches(); });
  py::class_<MelFeature, VectorFeatureStream, cref<MelFeature>>(m, "MelFeaturePtr")
      .def(py::init([](py::object mag, int pow_num, float rate, float low, float up, unsigned filter_num, unsigned version, const std::string& nm) {
             VectorFeatureStreamPtr sp = as_dstream(mag);
             return new MelFeature(sp, pow_num, rate, low, up, filter_num, version, nm);
           }), py::arg("mag"), py::arg("pow_num") = 0, py::arg("rate") = 16000.0f, py::arg("low") = 0.0f, py::arg("up") = 0.0f,
           py::arg("filter_num") = 30, py::arg("version") = 1, py::arg("nm") = "MelFFT")
      .def("read", [](MelFeature& f, const std::string& fn) { f.read(fn); }, py::arg("fileName"))
      .def("matrix", [](MelFeature& f, py::object out) { return matrix_of(f, f.size(), f.powN(), out); }, py::arg("matrix") = py::none())
      .def("set_block_frames", [](MelFeature& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](MelFeature& f) { return f.block_frames(); })
      .def("launches", [](MelFeature& f) { return f.launches(); });
  py::class_<LogFeature, VectorFloatFeatureStream, cref<LogFeature>>(m, "LogFeaturePtr")
      .def(py::init([](py::object mel, double mm, double a, bool sphinxFlooring, const std::string& nm) {
             VectorFeatureStreamPtr sp = as_dstream(mel);
             return new LogFeature(sp, mm, a, sphinxFlooring, nm);
           }), py::arg("mel"), py::arg("m") = 1.0, py::arg("a") = 1.0, py::arg("sphinxFlooring") = false, py::arg("nm") = "LogMel")
      .def("set_block_frames", [](LogFeature& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](LogFeature& f) { return f.block_frames(); })
      .def("launches", [](LogFeature& f) { return f.launches(); });
  py::class_<CepstralFeature, VectorFloatFeatureStream, cref<CepstralFeature>>(m, "CepstralFeaturePtr")
      .def(py::init([](py::object mel, unsigned ncep, int type, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(mel);
             return new CepstralFeature(sp, ncep, type, nm);
           }), py::arg("mel"), py::arg("ncep") = 13, py::arg("type") = 1, py::arg("nm") = "Cepstral")
      .def("matrix", [](CepstralFeature& f) { gsl_matrix* mm = f.matrix(); py::array a = dense_of(mm); gsl_matrix_free(mm); return a; })
      .def("set_block_frames", [](CepstralFeature& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](CepstralFeature& f) { return f.block_frames(); })
      .def("launches", [](CepstralFeature& f) { return f.launches(); });

  // ---- convolution/convolution.h (convolution/convolution.i:45-107); block_frames / set_block_frames / launches / plan are the engine's additions
  py::class_<OverlapAdd, VectorFloatFeatureStream, cref<OverlapAdd>>(m, "OverlapAddPtr")
      .def(py::init([](py::object samp, py::array_t<double, py::array::c_style | py::array::forcecast> impulse_response, unsigned fft_len,
                       const std::string& nm, long block_frames) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             GslVec h(impulse_response);
             return new OverlapAdd(sp, h.v, fft_len, nm, block_frames);
           }), py::arg("samp"), py::arg("impulse_response"), py::arg("fft_len") = 0, py::arg("nm") = "Overlap Add", py::arg("block_frames") = 0)
      .def("fftLen", &OverlapAdd::fftLen)
      .def("taps", [](OverlapAdd& f) { return f.taps(); })
      .def("plan", [](OverlapAdd& f) { int N, Lk, Bp, Q; f.plan(&N, &Lk, &Bp, &Q); return py::make_tuple(N, Lk, Bp, Q); })
      .def("set_block_frames", [](OverlapAdd& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](OverlapAdd& f) { return f.block_frames(); })
      .def("launches", [](OverlapAdd& f) { return f.launches(); });
  py::class_<OverlapSave, VectorFloatFeatureStream, cref<OverlapSave>>(m, "OverlapSavePtr")
      .def(py::init([](py::object samp, py::array_t<double, py::array::c_style | py::array::forcecast> impulse_response, const std::string& nm,
                       long block_frames) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             GslVec h(impulse_response);
             return new OverlapSave(sp, h.v, nm, block_frames);
           }), py::arg("samp"), py::arg("impulse_response"), py::arg("nm") = "Overlap Save", py::arg("block_frames") = 0)
      .def("taps", [](OverlapSave& f) { return f.taps(); })
      .def("plan", [](OverlapSave& f) { int N, Lk, Bp, Q; f.plan(&N, &Lk, &Bp, &Q); return py::make_tuple(N, Lk, Bp, Q); })
      .def("set_block_frames", [](OverlapSave& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](OverlapSave& f) { return f.block_frames(); })
      .def("launches", [](OverlapSave& f) { return f.launches(); });

  // ---- modulated/modulated.h
  py::class_<OverSampledDFTAnalysisBank, VectorComplexFeatureStream, cref<OverSampledDFTAnalysisBank>>(m, "OverSampledDFTAnalysisBankPtr")
      .def(py::init([](py::object samp, py::array_t<double, py::array::c_style | py::array::forcecast> prototype, unsigned M, unsigned mm,
                       unsigned r, unsigned dct, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             GslVec h(prototype);
             return new OverSampledDFTAnalysisBank(sp, h.v, M, mm, r, dct, nm);
           }), py::arg("samp"), py::arg("prototype"), py::arg("M"), py::arg("m"), py::arg("r"), py::arg("delay_compensation_type") = 0,
           py::arg("nm") = "OverSampledDFTAnalysisBank")
      .def("fftlen", &OverSampledDFTAnalysisBank::fftlen)
      .def("fftLen", &OverSampledDFTAnalysisBank::fftlen)
      .def("shiftlen", &OverSampledDFTAnalysisBank::shiftlen)
      .def("nBlocks", &OverSampledDFTAnalysisBank::nBlocks)
      .def("subSampRate", &OverSampledDFTAnalysisBank::subSampRate)
      .def("set_block_frames", &OverSampledDFTAnalysisBank::set_block_frames, py::arg("n"))
      .def("block_frames", &OverSampledDFTAnalysisBank::block_frames);
  py::class_<OverSampledDFTSynthesisBank, VectorFloatFeatureStream, cref<OverSampledDFTSynthesisBank>>(m, "OverSampledDFTSynthesisBankPtr")
      // source-less form (modulated/modulated.i:151-171): frames are pushed with input_source_vector(); registered first so that a
      // prototype array in the first position is not taken for a source object
      .def(py::init([](py::array_t<double, py::array::c_style | py::array::forcecast> prototype, unsigned M, unsigned mm, unsigned r,
                       unsigned dct, int gain_factor, const std::string& nm) {
             GslVec g(prototype);
             return new OverSampledDFTSynthesisBank(g.v, M, mm, r, dct, gain_factor, nm);
           }), py::arg("prototype"), py::arg("M"), py::arg("m"), py::arg("r") = 0, py::arg("delay_compensation_type") = 0,
           py::arg("gain_factor") = 1, py::arg("nm") = "OverSampledDFTSynthesisBank")
      .def(py::init([](py::object samp, py::array_t<double, py::array::c_style | py::array::forcecast> prototype, unsigned M, unsigned mm,
                       unsigned r, unsigned dct, int gain_factor, const std::string& nm) {
             VectorComplexFeatureStreamPtr sp = as_cstream(samp);
             GslVec g(prototype);
             return new OverSampledDFTSynthesisBank(sp, g.v, M, mm, r, dct, gain_factor, nm);
           }), py::arg("samp"), py::arg("prototype"), py::arg("M"), py::arg("m"), py::arg("r") = 0, py::arg("delay_compensation_type") = 0,
           py::arg("gain_factor") = 1, py::arg("nm") = "OverSampledDFTSynthesisBank")
      .def("input_source_vector", [](OverSampledDFTSynthesisBank& b, py::array_t<cd, py::array::c_style | py::array::forcecast> block) {
             GslCVec v(block); b.input_source_vector(v.v); }, py::arg("block"))
      .def("inputSourceVector", [](OverSampledDFTSynthesisBank& b, py::array_t<cd, py::array::c_style | py::array::forcecast> block) {
             GslCVec v(block); b.input_source_vector(v.v); }, py::arg("block"))
      .def("no_stream_feature", &OverSampledDFTSynthesisBank::no_stream_feature, py::arg("flag") = true)
      .def("doNotUseStreamFeature", &OverSampledDFTSynthesisBank::no_stream_feature, py::arg("flag") = true)
      .def("set_block_frames", &OverSampledDFTSynthesisBank::set_block_frames, py::arg("n"))
      .def("block_frames", &OverSampledDFTSynthesisBank::block_frames)
      // engine extension: the blocks the next calls of next() would return, as one float32 array [n][shiftlen] (n = 0: end of stream)
      .def("next_blocks", [](OverSampledDFTSynthesisBank& b, long max_blocks) {
             const float* p = NULL;
             const long n = b.next_blocks(max_blocks, &p);
             py::array_t<float> a({(py::ssize_t)n, (py::ssize_t)b.size()});
             if (n > 0) memcpy(a.mutable_data(), p, sizeof(float) * (size_t)n * b.size());
             return a;
           }, py::arg("max_blocks") = 0);
  // the PR banks, the windowed FFT bank, DelayFeature and get_window (modulated/modulated.i:46-86, :194-305, :477-478);
  // block_frames / set_block_frames / launches are the engine's additions
  py::class_<NormalFFTAnalysisBank, VectorComplexFeatureStream, cref<NormalFFTAnalysisBank>>(m, "NormalFFTAnalysisBankPtr")
      .def(py::init([](py::object samp, unsigned fftLen, unsigned r, unsigned window_type, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             return new NormalFFTAnalysisBank(sp, fftLen, r, window_type, nm);
           }), py::arg("samp"), py::arg("fftLen"), py::arg("r") = 1, py::arg("window_type") = 1, py::arg("nm") = "NormalFFTAnalysisBank")
      .def("fftlen", &NormalFFTAnalysisBank::fftlen)
      .def("fftLen", &NormalFFTAnalysisBank::fftlen)
      .def("set_block_frames", [](NormalFFTAnalysisBank& b, long n) { b.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](NormalFFTAnalysisBank& b) { return b.block_frames(); })
      .def("launches", [](NormalFFTAnalysisBank& b) { return b.launches(); });
  py::class_<PerfectReconstructionFFTAnalysisBank, VectorComplexFeatureStream, cref<PerfectReconstructionFFTAnalysisBank>>(m, "PerfectReconstructionFFTAnalysisBankPtr")
      .def(py::init([](py::object samp, py::array_t<double, py::array::c_style | py::array::forcecast> prototype, unsigned M, unsigned mm,
                       unsigned r, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(samp);
             GslVec h(prototype);
             return new PerfectReconstructionFFTAnalysisBank(sp, h.v, M, mm, r, nm);
           }), py::arg("samp"), py::arg("prototype"), py::arg("M") = 256, py::arg("m") = 3, py::arg("r") = 0,
           py::arg("nm") = "PerfectReconstructionFFTAnalysisBankFloat")
      .def("polyphase", &PerfectReconstructionFFTAnalysisBank::polyphase, py::arg("m"), py::arg("n"))
      .def("fftLen", &PerfectReconstructionFFTAnalysisBank::fftLen)
      .def("nBlocks", &PerfectReconstructionFFTAnalysisBank::nBlocks)
      .def("subSampRate", &PerfectReconstructionFFTAnalysisBank::subSampRate)
      .def("set_block_frames", [](PerfectReconstructionFFTAnalysisBank& b, long n) { b.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](PerfectReconstructionFFTAnalysisBank& b) { return b.block_frames(); })
      .def("launches", [](PerfectReconstructionFFTAnalysisBank& b) { return b.launches(); });
  py::class_<PerfectReconstructionFFTSynthesisBank, VectorFloatFeatureStream, cref<PerfectReconstructionFFTSynthesisBank>>(m, "PerfectReconstructionFFTSynthesisBankPtr")
      // source-less form (modulated/modulated.i:250-251), registered first so that a prototype array in the first position is not
      // taken for a source object
      .def(py::init([](py::array_t<double, py::array::c_style | py::array::forcecast> prototype, unsigned M, unsigned mm, unsigned r,
                       const std::string& nm) {
             GslVec g(prototype);
             return new PerfectReconstructionFFTSynthesisBank(g.v, M, mm, r, nm);
           }), py::arg("prototype"), py::arg("M"), py::arg("m"), py::arg("r") = 0, py::arg("nm") = "PerfectReconstructionFFTSynthesisBF")
      .def(py::init([](py::object samp, py::array_t<double, py::array::c_style | py::array::forcecast> prototype, unsigned M, unsigned mm,
                       unsigned r, const std::string& nm) {
             VectorComplexFeatureStreamPtr sp = as_cstream(samp);
             GslVec g(prototype);
             return new PerfectReconstructionFFTSynthesisBank(sp, g.v, M, mm, r, nm);
           }), py::arg("samp"), py::arg("prototype"), py::arg("M"), py::arg("m"), py::arg("r") = 0,
           py::arg("nm") = "PerfectReconstructionFFTSynthesisBank")
      .def("polyphase", &PerfectReconstructionFFTSynthesisBank::polyphase, py::arg("m"), py::arg("n"))
      .def("set_block_frames", &PerfectReconstructionFFTSynthesisBank::set_block_frames, py::arg("n"))
      .def("block_frames", &PerfectReconstructionFFTSynthesisBank::block_frames)
      .def("launches", &PerfectReconstructionFFTSynthesisBank::launches);
  py::class_<DelayFeature, VectorComplexFeatureStream, cref<DelayFeature>>(m, "DelayFeaturePtr")
      .def(py::init([](py::object samp, float time_delay, const std::string& nm) {
             VectorComplexFeatureStreamPtr sp = as_cstream(samp);
             return new DelayFeature(sp, time_delay, nm);
           }), py::arg("samp"), py::arg("time_delay") = 0.0f, py::arg("nm") = "DelayFeature")
      .def("set_time_delay", [](DelayFeature& f, double time_delay) { f.set_time_delay((float)time_delay); }, py::arg("time_delay"));
  m.def("get_window", [](unsigned winType, unsigned winLen) {
          gsl_vector* w = get_window(winType, winLen);
          py::array_t<double> a((py::ssize_t)w->size);
          memcpy(a.mutable_data(), w->data, sizeof(double) * w->size);
          gsl_vector_free(w);
          return a;
        }, py::arg("winType"), py::arg("winLen"));

  // ---- beamformer/beamformer.h
  py::class_<SnapShotArray, cref<SnapShotArray>>(m, "SnapShotArrayPtr")
      .def(py::init([](unsigned fftLn, unsigned nChn) { return new SnapShotArray(fftLn, nChn); }), py::arg("fftLn"), py::arg("nChn"))
      .def("fftLen", &SnapShotArray::fftLen)
      .def("nChan", &SnapShotArray::nChan)
      .def("set_samples", [](SnapShotArray& a, py::array_t<cd, py::array::c_style | py::array::forcecast> s, unsigned chanX) {
             if ((unsigned)s.size() != a.fftLen()) throw jdimension_error("sample vector has %d entries, fftLen is %d", (int)s.size(), (int)a.fftLen());
             GslCVec v(s); a.set_samples(v.v, chanX); })
      .def("set_snapshots", [](SnapShotArray& a, py::array_t<cd, py::array::c_style | py::array::forcecast> s, unsigned fbinX) {
             GslCVec v(s); a.set_snapshots(v.v, fbinX); })
      .def("newSample", [](SnapShotArray& a, py::array_t<cd, py::array::c_style | py::array::forcecast> s, unsigned chanX) {
             if ((unsigned)s.size() != a.fftLen()) throw jdimension_error("sample vector has %d entries, fftLen is %d", (int)s.size(), (int)a.fftLen());
             GslCVec v(s); a.set_samples(v.v, chanX); })
      .def("getSnapShot", [](SnapShotArray& a, unsigned fbinX) { return copy_of(a.snapshot(fbinX)); })
      .def("update", [](SnapShotArray& a) { a.update(); })
      .def("zero", [](SnapShotArray& a) { a.zero(); })
      .def("snapshot", [](SnapShotArray& a, unsigned fbinX) { return copy_of(a.snapshot(fbinX)); });
  py::class_<SpectralMatrixArray, SnapShotArray, cref<SpectralMatrixArray>>(m, "SpectralMatrixArrayPtr")
      .def(py::init([](unsigned fftLn, unsigned nChn, float forgetFact) { return new SpectralMatrixArray(fftLn, nChn, forgetFact); }),
           py::arg("fftLn"), py::arg("nChn"), py::arg("forgetFact") = 0.95f)
      .def("matrix_f", [](SpectralMatrixArray& a, unsigned idx) { return copy_of(a.matrix_f(idx)); })
      .def("getSpecMatrix", [](SpectralMatrixArray& a, unsigned idx) { return copy_of(a.matrix_f(idx)); });

  py::class_<SubbandBeamformer, VectorComplexFeatureStream, cref<SubbandBeamformer>>(m, "SubbandBeamformer")
      .def("set_channel", [](SubbandBeamformer& b, py::object chan) { VectorComplexFeatureStreamPtr p = as_cstream(chan); b.set_channel(p); })
      .def("setChannel", [](SubbandBeamformer& b, py::object chan) { VectorComplexFeatureStreamPtr p = as_cstream(chan); b.set_channel(p); })
      .def("_device_snapshots_info", [](SubbandBeamformer& b) {      // (device pointer, K, N, T) of the complex64 [K][N][T] snapshot block
             void* p = b.device_snapshots();
             return py::make_tuple((size_t)reinterpret_cast<uintptr_t>(p), (long)(b.fftLen() / 2 + 1), (long)b.chanN(), b.num_frames()); })
      .def("clear_channel", [](SubbandBeamformer& b) { b.clear_channel(); })
      .def("clearChannel", [](SubbandBeamformer& b) { b.clear_channel(); })
      .def("chan_num", &SubbandBeamformer::chanN)
      .def("chanN", &SubbandBeamformer::chanN)
      .def("fftlen", &SubbandBeamformer::fftLen)
      .def("fftLen", &SubbandBeamformer::fftLen)
      .def("dim", &SubbandBeamformer::dim)
      .def("want_snapshots", &SubbandBeamformer::want_snapshots)   // every block from now on brings its snapshots along (staged path)
      .def("i16_stream", &SubbandBeamformer::i16_stream)   // the current stream's samples go up as 16-bit PCM (every source holds it)
      .def("snapshots_materialised", &SubbandBeamformer::snapshots_materialised)   // the current block's snapshots exist on the device
      .def("num_frames", &SubbandBeamformer::num_frames)                 // frames of the current block of snapshots
      .def("chunk_base", &SubbandBeamformer::chunk_base)                 // stream index of its first frame
      .def("set_block_frames", &SubbandBeamformer::set_block_frames, py::arg("n"))
      .def("block_frames", &SubbandBeamformer::block_frames)
      .def("set_block_quantum", &SubbandBeamformer::set_block_quantum, py::arg("q"))
      .def("block_quantum", &SubbandBeamformer::block_quantum)
      .def("is_half_band_shift", &SubbandBeamformer::is_half_band_shift)
      .def("snapshot_array_f", [](SubbandBeamformer& b, unsigned fbinX) { return copy_of(b.snapshot_array_f(fbinX)); })
      .def("snapshot_array", [](SubbandBeamformer& b) { SnapShotArrayPtr a = b.snapshot_array(); return cref<SnapShotArray>(a.operator->()); })
      .def("getSnapShotArray", [](SubbandBeamformer& b) { SnapShotArrayPtr a = b.snapshot_array(); return cref<SnapShotArray>(a.operator->()); });

  // BeamformerWeights (beamformer.h:26-97), owned by its beamformer node: whole-array views of the reference's per-bin accessors
  py::class_<BeamformerWeights, std::unique_ptr<BeamformerWeights, py::nodelete>>(m, "BeamformerWeights")
      .def("fftLen", &BeamformerWeights::fftLen)
      .def("chanN", &BeamformerWeights::chanN)
      .def("NC", &BeamformerWeights::NC)
      .def("isHalfBandShift", &BeamformerWeights::isHalfBandShift)
      .def("wq_f", [](BeamformerWeights& w, unsigned fbinX) { if (fbinX >= w.fftLen()) throw jindex_error("bin %d of %d", (int)fbinX, (int)w.fftLen()); return copy_of(w.wq_f(fbinX)); })
      .def("wl_f", [](BeamformerWeights& w, unsigned fbinX) { if (fbinX >= w.fftLen()) throw jindex_error("bin %d of %d", (int)fbinX, (int)w.fftLen()); return copy_of(w.wl_f(fbinX)); })
      .def_property_readonly("wq", [](BeamformerWeights& w) {
             py::array_t<cd> a({(py::ssize_t)w.fftLen(), (py::ssize_t)w.chanN()});
             memcpy(static_cast<void*>(a.mutable_data()), w.wq_v.data(), sizeof(cd) * w.wq_v.size()); return a; })
      .def_property_readonly("wl", [](BeamformerWeights& w) {
             py::array_t<cd> a({(py::ssize_t)w.fftLen(), (py::ssize_t)w.chanN()});
             memcpy(static_cast<void*>(a.mutable_data()), w.wl_v.data(), sizeof(cd) * w.wl_v.size()); return a; })
      .def_property_readonly("ta", [](BeamformerWeights& w) {
             py::array_t<cd> a({(py::ssize_t)w.fftLen(), (py::ssize_t)w.chanN()});
             memcpy(static_cast<void*>(a.mutable_data()), w.ta_v.data(), sizeof(cd) * w.ta_v.size()); return a; })
      .def_property_readonly("wa", [](BeamformerWeights& w) {
             py::array_t<cd> a({(py::ssize_t)w.fftLen(), (py::ssize_t)(w.chanN() - w.NC())});
             memcpy(static_cast<void*>(a.mutable_data()), w.wa_v.data(), sizeof(cd) * w.wa_v.size()); return a; })
      // the reference's auto / cross spectral densities of bin fbinX as an N x N matrix (entry [i][j], i <= j; rebuilt on demand)
      .def("CSDs", [](BeamformerWeights& w, unsigned fbinX) {
             if (fbinX >= w.fftLen()) throw jindex_error("bin %d of %d", (int)fbinX, (int)w.fftLen());
             gsl_vector_complex** c = w.CSDs();
             py::array_t<cd> a({(py::ssize_t)w.chanN(), (py::ssize_t)w.chanN()});
             memcpy(static_cast<void*>(a.mutable_data()), c[fbinX]->data, sizeof(cd) * w.chanN() * w.chanN()); return a; }, py::arg("fbinX"))
      .def("wp1", [](BeamformerWeights& w) { return copy_of(w.wp1()); })
      .def_property_readonly("B", [](BeamformerWeights& w) {
             py::array_t<cd> a({(py::ssize_t)w.fftLen(), (py::ssize_t)w.chanN(), (py::ssize_t)(w.chanN() - w.NC())});
             memcpy(static_cast<void*>(a.mutable_data()), w.B_v.data(), sizeof(cd) * w.B_v.size()); return a; });

  py::class_<SubbandDS, SubbandBeamformer, cref<SubbandDS>>(m, "SubbandDSPtr")
      .def(py::init([](unsigned fftlen, bool half_band_shift, const std::string& nm) { return new SubbandDS(fftlen, half_band_shift, nm); }),
           py::arg("fftlen") = 512, py::arg("half_band_shift") = false, py::arg("nm") = "SubbandDS")
      .def("calc_array_manifold_vectors", [](SubbandDS& b, float fs, py::array_t<double, py::array::c_style | py::array::forcecast> d) {
             GslVec v(d); b.calc_array_manifold_vectors(fs, v.v); }, py::arg("samplerate"), py::arg("delays"))
      .def("calc_array_manifold_vectors_2", [](SubbandDS& b, float fs, py::array_t<double, py::array::c_style | py::array::forcecast> dt,
                                               py::array_t<double, py::array::c_style | py::array::forcecast> dj) {
             GslVec a(dt), c(dj); b.calc_array_manifold_vectors_2(fs, a.v, c.v); })
      .def("calc_array_manifold_vectors_n", [](SubbandDS& b, float fs, py::array_t<double, py::array::c_style | py::array::forcecast> dt,
                                               py::array_t<double, py::array::c_style | py::array::forcecast> djs, unsigned NC) {
             GslVec a(dt); GslMat c(djs); b.calc_array_manifold_vectors_n(fs, a.v, c.m, NC); }, py::arg("samplerate"), py::arg("delays_t"), py::arg("delays_js"), py::arg("NC") = 2)
      .def("get_weights", [](SubbandDS& b, unsigned fbinX) { return copy_of(b.get_weights(fbinX)); })
      .def("getWeights", [](SubbandDS& b, unsigned fbinX) { return copy_of(b.get_weights(fbinX)); })
      .def("beamformer_weight_object", [](SubbandDS& b, unsigned srcX) -> py::object {
             BeamformerWeights* w = b.beamformer_weight_object(srcX);
             return w ? py::cast(w, py::return_value_policy::reference) : py::object(py::none()); }, py::arg("srcX") = 0, py::keep_alive<0, 1>())
      // the block protocol a batching consumer uses (modulated/modulated.h BlockSource), under the names of the Python-side protocol
      .def("device_block", [](SubbandDS& b) { return block_of(b); })
      .def("fused_path", &SubbandDS::fused_path)   // the node's blocks come from the fused analysis -> apply kernel
      .def("_output_version", [](SubbandDS& b) { return b.block_version(); })
      .def("_advance_to", [](SubbandDS& b, long idx) { b.advance_to(idx); })
      .def("_block_base", [](SubbandDS& b) { return b.block_base(); })
      .def("_next_block", [](SubbandDS& b) { return b.next_block(); });

  py::class_<SubbandGSC, SubbandDS, cref<SubbandGSC>>(m, "SubbandGSCPtr")
      .def(py::init([](unsigned fftlen, bool half_band_shift, const std::string& nm) { return new SubbandGSC(fftlen, half_band_shift, nm); }),
           py::arg("fftlen") = 512, py::arg("half_band_shift") = false, py::arg("nm") = "SubbandGSC")
      .def("normalize_weight", &SubbandGSC::normalize_weight)
      .def("calc_gsc_weights", [](SubbandGSC& b, float fs, py::array_t<double, py::array::c_style | py::array::forcecast> d) { GslVec v(d); b.calc_gsc_weights(fs, v.v); })
      .def("calc_gsc_weights_2", [](SubbandGSC& b, float fs, py::array_t<double, py::array::c_style | py::array::forcecast> dt,
                                    py::array_t<double, py::array::c_style | py::array::forcecast> dj) { GslVec a(dt), c(dj); b.calc_gsc_weights_2(fs, a.v, c.v); })
      .def("calc_gsc_weights_n", [](SubbandGSC& b, float fs, py::array_t<double, py::array::c_style | py::array::forcecast> dt,
                                    py::array_t<double, py::array::c_style | py::array::forcecast> djs, unsigned NC) {
             GslVec a(dt); GslMat c(djs); b.calc_gsc_weights_n(fs, a.v, c.m, NC); }, py::arg("samplerate"), py::arg("delays_t"), py::arg("delays_js"), py::arg("NC") = 2)
      .def("set_active_weights_f", [](SubbandGSC& b, unsigned fbinX, py::array_t<double, py::array::c_style | py::array::forcecast> packed) {
             GslVec v(packed); b.set_active_weights_f(fbinX, v.v); })
      .def("set_quiescent_weights_f", [](SubbandGSC& b, unsigned fbinX, py::array_t<cd, py::array::c_style | py::array::forcecast> wq) {
             GslCVec v(wq); b.set_quiescent_weights_f(fbinX, v.v); })
      .def("zero_active_weights", &SubbandGSC::zero_active_weights)
      .def("write_fir_coeff", [](SubbandGSC& b, const std::string& fn, unsigned winType) { return b.write_fir_coeff(fn, winType); }, py::arg("fn"), py::arg("winType") = 1)
      .def("blocking_matrix", [](SubbandGSC& b, unsigned srcX, unsigned fbinX) { return copy_of(b.blocking_matrix(srcX, fbinX)); });

  py::class_<SubbandGSCRLS, SubbandGSC, cref<SubbandGSCRLS>>(m, "SubbandGSCRLSPtr")
      .def(py::init([](unsigned fftlen, bool half_band_shift, float mu, float sigma2, const std::string& nm) {
             return new SubbandGSCRLS(fftlen, half_band_shift, mu, sigma2, nm); }),
           py::arg("fftlen") = 512, py::arg("half_band_shift") = false, py::arg("mu") = 0.9f, py::arg("sigma2") = 0.0f, py::arg("nm") = "SubbandGSCRLS")
      .def("init_precision_matrix", &SubbandGSCRLS::init_precision_matrix, py::arg("sigma2") = 0.01f)
      .def("set_precision_matrix", [](SubbandGSCRLS& b, unsigned fbinX, py::array_t<cd, py::array::c_style | py::array::forcecast> Pz) {
             GslCMat M(Pz); b.set_precision_matrix(fbinX, M.m); })
      .def("update_active_weight_vecotrs", &SubbandGSCRLS::update_active_weight_vecotrs)
      .def("set_quadratic_constraint", &SubbandGSCRLS::set_quadratic_constraint, py::arg("alpha"), py::arg("qctype") = 1);

  py::class_<SubbandMVDR, SubbandDS, cref<SubbandMVDR>>(m, "SubbandMVDRPtr")
      .def(py::init([](unsigned fftlen, bool half_band_shift, const std::string& nm) { return new SubbandMVDR(fftlen, half_band_shift, nm); }),
           py::arg("fftlen") = 512, py::arg("half_band_shift") = false, py::arg("nm") = "SubbandMVDR")
      .def("calc_mvdr_weights", &SubbandMVDR::calc_mvdr_weights, py::arg("samplerate"), py::arg("threshold") = 1.0E-8f, py::arg("calc_inverse_matrix") = true)
      .def("mvdr_weights", [](SubbandMVDR& b, unsigned fbinX) { return copy_of(b.mvdr_weights(fbinX)); })
      .def("set_noise_spatial_spectral_matrix", [](SubbandMVDR& b, unsigned fbinX, py::array_t<cd, py::array::c_style | py::array::forcecast> Rnn) {
             GslCMat M(Rnn); return b.set_noise_spatial_spectral_matrix(fbinX, M.m); })
      .def("noise_spatial_spectral_matrix", [](SubbandMVDR& b, unsigned fbinX) -> py::object {      // None while no matrix is set (the reference returns NULL)
             const gsl_matrix_complex* m = b.noise_spatial_spectral_matrix(fbinX); return m ? py::object(copy_of(m)) : py::object(py::none()); })
      .def("set_diffuse_noise_model", [](SubbandMVDR& b, py::array_t<double, py::array::c_style | py::array::forcecast> mpos, float fs, float sspeed) {
             GslMat M(mpos); return b.set_diffuse_noise_model(M.m, fs, sspeed); }, py::arg("mic_positions"), py::arg("samplerate"), py::arg("sspeed") = 343740.0f)
      .def("set_all_diagonal_loading", &SubbandMVDR::set_all_diagonal_loading)
      .def("set_diagonal_looading", &SubbandMVDR::set_diagonal_looading)
      .def("divide_all_nondiagonal_elements", &SubbandMVDR::divide_all_nondiagonal_elements)
      .def("divide_nondiagonal_elements", &SubbandMVDR::divide_nondiagonal_elements)
      .def("identity_fallbacks", &SubbandMVDR::identity_fallbacks)
      .def("set_svd_rule", &SubbandMVDR::set_svd_rule, py::arg("rule"))
      .def("svd_rule", &SubbandMVDR::svd_rule)
      .def("csvdc_not_converged", &SubbandMVDR::csvdc_not_converged);

  py::class_<SubbandMVDRGSC, SubbandMVDR, cref<SubbandMVDRGSC>>(m, "SubbandMVDRGSCPtr")
      .def(py::init([](unsigned fftlen, bool half_band_shift, const std::string& nm) { return new SubbandMVDRGSC(fftlen, half_band_shift, nm); }),
           py::arg("fftlen") = 512, py::arg("half_band_shift") = false, py::arg("nm") = "SubbandMVDR")
      .def("normalize_weight", &SubbandMVDRGSC::normalize_weight)
      .def("set_active_weights_f", [](SubbandMVDRGSC& b, unsigned fbinX, py::array_t<double, py::array::c_style | py::array::forcecast> packed) {
             GslVec v(packed); b.set_active_weights_f(fbinX, v.v); })
      .def("zero_active_weights", &SubbandMVDRGSC::zero_active_weights)
      .def("calc_blocking_matrix1", [](SubbandMVDRGSC& b, float fs, py::array_t<double, py::array::c_style | py::array::forcecast> d) {
             GslVec v(d); return b.calc_blocking_matrix1(fs, v.v); })
      .def("calc_blocking_matrix2", &SubbandMVDRGSC::calc_blocking_matrix2)
      .def("upgrade_blocking_matrix", &SubbandMVDRGSC::upgrade_blocking_matrix)
      .def("blocking_matrix_output", [](SubbandMVDRGSC& b, int outChanX) { return copy_of(b.blocking_matrix_output(outChanX)); }, py::arg("outChanX") = 0);

  // ---- DOA estimation (beamformer.i:674-757)
  {
    py::class_<DOAEstimatorSRPBase, std::shared_ptr<DOAEstimatorSRPBase>> base(m, "DOAEstimatorSRPBasePtr");
    base.def(py::init([](unsigned nBest, unsigned fbinMax) { return std::make_shared<DOAEstimatorSRPBase>(nBest, fbinMax); }),
             py::arg("nBest"), py::arg("fbinMax"));
    def_srp_base<DOAEstimatorSRPBase>(base);
    // (the node base is the class's SECOND base, as in the reference: its subobject does not start where the object does)
    py::class_<DOAEstimatorSRPDSBLA, SubbandDS, cref<DOAEstimatorSRPDSBLA>> dsb(m, "DOAEstimatorSRPDSBLAPtr", py::multiple_inheritance());
    dsb.def(py::init([](unsigned nBest, unsigned samplerate, unsigned fftlen, const std::string& nm) {
              return new DOAEstimatorSRPDSBLA(nBest, samplerate, fftlen, nm); }),
            py::arg("nBest"), py::arg("samplerate"), py::arg("fftlen"), py::arg("nm") = "DOAEstimatorSRPDSBLAPtr");
    def_srp_base<DOAEstimatorSRPDSBLA>(dsb);
    auto geom = [](DOAEstimatorSRPDSBLA& e, py::array_t<double, py::array::c_style | py::array::forcecast> positions) {
      GslVec v(positions); e.set_array_geometry(v.v); };
    dsb.def("set_array_geometry", geom, py::arg("positions")).def("setArrayGeometry", geom, py::arg("positions"));
  }

  // ---- postfilter/postfilter.h
  py::class_<ZelinskiPostFilter, VectorComplexFeatureStream, cref<ZelinskiPostFilter>>(m, "ZelinskiPostFilterPtr")
      .def(py::init([](py::object output, unsigned fftlen, double alpha, int type, int min_frames, const std::string& nm) {
             VectorComplexFeatureStreamPtr p = as_cstream(output);
             return new ZelinskiPostFilter(p, fftlen, alpha, type, min_frames, nm);
           }), py::arg("output"), py::arg("fftlen"), py::arg("alpha") = 0.6, py::arg("type") = 2, py::arg("min_frames") = 0, py::arg("nm") = "ZelinskPostFilter")
      .def("set_beamformer", [](ZelinskiPostFilter& f, SubbandDS* bf) { SubbandDSPtr p(bf); f.set_beamformer(p); })
      .def("setBeamformer", [](ZelinskiPostFilter& f, SubbandDS* bf) { SubbandDSPtr p(bf); f.set_beamformer(p); })
      .def("set_snapshot_array", [](ZelinskiPostFilter& f, SnapShotArray* a) { SnapShotArrayPtr p(a); f.set_snapshot_array(p); }, py::arg("snapShotArray"))
      .def("setSnapShotArray", [](ZelinskiPostFilter& f, SnapShotArray* a) { SnapShotArrayPtr p(a); f.set_snapshot_array(p); }, py::arg("snapShotArray"))
      .def("set_array_manifold_vector", [](ZelinskiPostFilter& f, unsigned fbinX, py::array_t<cd, py::array::c_style | py::array::forcecast> v, bool halfBandShift, unsigned NC) {
             GslCVec g(v); f.set_array_manifold_vector(fbinX, g.v, halfBandShift, NC); },
           py::arg("fbinX"), py::arg("arrayManifoldVector"), py::arg("halfBandShift"), py::arg("NC") = 1)
      .def("setArrayManifoldVector", [](ZelinskiPostFilter& f, unsigned fbinX, py::array_t<cd, py::array::c_style | py::array::forcecast> v, bool halfBandShift, unsigned NC) {
             GslCVec g(v); f.set_array_manifold_vector(fbinX, g.v, halfBandShift, NC); },
           py::arg("fbinX"), py::arg("arrayManifoldVector"), py::arg("halfBandShift"), py::arg("NC") = 1)
      .def("weights_object", [](py::object self) -> py::object {            // bf_weights_ (postfilter.h:104); None before any weights exist
             ZelinskiPostFilter& f = self.cast<ZelinskiPostFilter&>();
             BeamformerWeights* w = f.weights_object();
             // the handle keeps the post-filter alive (reference_internal): the filter owns the object it made for
             // set_array_manifold_vector(), and keeps its beamformer -- the owner otherwise -- alive itself
             return w ? py::cast(w, py::return_value_policy::reference_internal, self) : py::none(); })
      .def("getPostFilterWeights", [](ZelinskiPostFilter& f) { return copy_of(f.postfilter_weights()); })
      .def("postfilter_weights", [](ZelinskiPostFilter& f) { return copy_of(f.postfilter_weights()); })
      .def("device_block", [](ZelinskiPostFilter& f) { return block_of(f); })
      .def("_output_version", [](ZelinskiPostFilter& f) { return f.block_version(); })
      .def("_advance_to", [](ZelinskiPostFilter& f, long idx) { f.advance_to(idx); })
      .def("_block_base", [](ZelinskiPostFilter& f) { return f.block_base(); })
      .def("_next_block", [](ZelinskiPostFilter& f) { return f.next_block(); });
  py::class_<McCowanPostFilter, ZelinskiPostFilter, cref<McCowanPostFilter>>(m, "McCowanPostFilterPtr")
      .def(py::init([](py::object output, unsigned fftlen, double alpha, int type, int min_frames, float threshold, const std::string& nm) {
             VectorComplexFeatureStreamPtr p = as_cstream(output);
             return new McCowanPostFilter(p, fftlen, alpha, type, min_frames, threshold, nm);
           }), py::arg("output"), py::arg("fftlen"), py::arg("alpha") = 0.6, py::arg("type") = 2, py::arg("min_frames") = 0, py::arg("threshold") = 0.99f,
           py::arg("nm") = "McCowanPostFilter")
      .def("set_diffuse_noise_model", [](McCowanPostFilter& f, py::array_t<double, py::array::c_style | py::array::forcecast> mpos, double fs, double sspeed) {
             GslMat M(mpos); return f.set_diffuse_noise_model(M.m, fs, sspeed); }, py::arg("mic_positions"), py::arg("samplerate"), py::arg("sspeed") = 343740.0)
      .def("set_noise_spatial_spectral_matrix", [](McCowanPostFilter& f, unsigned fbinX, py::array_t<cd, py::array::c_style | py::array::forcecast> Rnn) {
             GslCMat M(Rnn); return f.set_noise_spatial_spectral_matrix(fbinX, M.m); })
      .def("noise_spatial_spectral_matrix", [](McCowanPostFilter& f, unsigned fbinX) -> py::object {
             const gsl_matrix_complex* m = f.noise_spatial_spectral_matrix(fbinX); return m ? py::object(copy_of(m)) : py::object(py::none()); })
      .def("set_all_diagonal_loading", &McCowanPostFilter::set_all_diagonal_loading)
      .def("set_diagonal_looading", &McCowanPostFilter::set_diagonal_looading)
      .def("divide_nondiagonal_elements", &McCowanPostFilter::divide_nondiagonal_elements)
      .def("divide_all_nondiagonal_elements", &McCowanPostFilter::divide_all_nondiagonal_elements)
      .def("setAllLevelsOfDiagonalLoading", &McCowanPostFilter::set_all_diagonal_loading)
      .def("setLevelOfDiagonalLoading", &McCowanPostFilter::set_diagonal_looading)
      .def("divideNonDiagonalElements", &McCowanPostFilter::divide_nondiagonal_elements)
      .def("divideAllNonDiagonalElements", &McCowanPostFilter::divide_all_nondiagonal_elements)
      .def("setNoiseSpatialSpectralMatrix", [](McCowanPostFilter& f, unsigned fbinX, py::array_t<cd, py::array::c_style | py::array::forcecast> Rnn) {
             GslCMat M(Rnn); return f.set_noise_spatial_spectral_matrix(fbinX, M.m); })
      .def("getNoiseSpatialSpectralMatrix", [](McCowanPostFilter& f, unsigned fbinX) { return copy_of(f.noise_spatial_spectral_matrix(fbinX)); })
      .def("set_svd_rule", [](McCowanPostFilter& f, const std::string& rule) { f.set_svd_rule(rule); }, py::arg("rule"))
      .def("svd_rule", [](McCowanPostFilter& f) { return std::string(f.svd_rule()); });
  py::class_<LefkimmiatisPostFilter, McCowanPostFilter, cref<LefkimmiatisPostFilter>>(m, "LefkimmiatisPostFilterPtr")
      .def(py::init([](py::object output, unsigned fftlen, double min_sv, unsigned fbin_x1, double alpha, int type, int min_frames,
                       float threshold, const std::string& nm) {
             VectorComplexFeatureStreamPtr p = as_cstream(output);
             return new LefkimmiatisPostFilter(p, fftlen, min_sv, fbin_x1, alpha, type, min_frames, threshold, nm);
           }), py::arg("output"), py::arg("fftlen"), py::arg("min_sv") = 1.0E-8, py::arg("fbin_x1") = 0, py::arg("alpha") = 0.6, py::arg("type") = 2,
           py::arg("min_frames") = 0, py::arg("threshold") = 0.99f, py::arg("nm") = "LefkimmiatisPostFilter")
      .def("calc_inverse_noise_spatial_spectral_matrix", &LefkimmiatisPostFilter::calc_inverse_noise_spatial_spectral_matrix);

  // ---- many utterance graphs advanced as one launch (beamformer/beamformer.h, SubbandGraphPool)
  py::class_<SubbandGraphPool, cref<SubbandGraphPool>>(m, "SubbandGraphPoolPtr")
      .def(py::init([]() { return new SubbandGraphPool(); }))
      .def("add", [](SubbandGraphPool& p, SubbandDS& bf, OverSampledDFTSynthesisBank& syn) {
             SubbandDSPtr b(&bf); OverSampledDFTSynthesisBankPtr s(&syn); p.add(b, s); }, py::arg("beamformer"), py::arg("synthesis"))
      .def("size", &SubbandGraphPool::size)
      .def("__len__", &SubbandGraphPool::size)
      .def("rounds", &SubbandGraphPool::rounds)
      .def("is_end", &SubbandGraphPool::is_end, py::arg("g"))
      // graph g's block of the last next() / next_round() (a view of the pool's buffer); None when that call had none for it
      .def("output", [](py::object self, unsigned g) -> py::object {
             const gsl_vector_float* v = self.cast<SubbandGraphPool&>().output(g);
             return v ? py::object(view(v, self)) : py::object(py::none()); }, py::arg("g"))
      .def("reset", &SubbandGraphPool::reset)
      // one output block per graph: a list with a numpy view of the pool's own buffer per graph, None for a graph that has ended;
      // StopIteration when every graph has ended
      .def("next", [](py::object self) {
             SubbandGraphPool& p = self.cast<SubbandGraphPool&>();
             bool ok; { py::gil_scoped_release rel; ok = p.next(); }
             if (!ok) throw py::stop_iteration();
             py::list out;
             for (unsigned g = 0; g < p.size(); g++) { const gsl_vector_float* v = p.output(g); if (v) out.append(view(v, self)); else out.append(py::none()); }
             return out; })
      .def("__next__", [](py::object self) { return self.attr("next")(); })
      .def("__iter__", [](py::object self) { self.attr("reset")(); return self; })
      // engine extension: a round at a time -- a list with one float32 array [n_g][shiftlen] per graph (n_g = 0: none in this round),
      // None when every graph has ended
      .def("next_round", [](SubbandGraphPool& p) -> py::object {
             bool ok; { py::gil_scoped_release rel; ok = p.next_round(); }
             if (!ok) return py::none();
             py::list out;
             for (unsigned g = 0; g < p.size(); g++) {
               const float* q = NULL;
               const long n = p.round_blocks(g, &q);
               const py::ssize_t D = n > 0 ? (py::ssize_t)p.output(g)->size : 0;
               py::array_t<float> a({(py::ssize_t)n, D});
               if (n > 0) memcpy(a.mutable_data(), q, sizeof(float) * (size_t)n * (size_t)D);
               out.append(a);
             }
             return out; });
  m.def("node_synchronize", []() { btk_node_synchronize(); });     // wait for everything this thread's nodes have launched
  m.def("node_alloc_counts", []() { long d = 0, h = 0; btk_node_alloc_counts(&d, &h); return py::make_tuple(d, h); });   // (device, pinned) allocation calls so far
  m.def("node_live_device_blocks", []() { return btk_node_live_device_blocks(); });   // device blocks the nodes hold right now
  m.def("node_d2h_bytes", []() { return btk_node_d2h_bytes(); });              // bytes copied device -> host by the nodes since the last reset
  m.def("node_d2h_bytes_reset", []() { btk_node_d2h_bytes_reset(); });

  // ---- dereverberation/dereverberation.h
  py::class_<MultiChannelWPEDereverberation, cref<MultiChannelWPEDereverberation>>(m, "MultiChannelWPEDereverberationPtr")
      .def(py::init([](unsigned subbands_num, unsigned channels_num, unsigned lower_num, unsigned upper_num, unsigned iterations_num, double load_db,
                       double band_width, double diagonal_bias, double samplerate) {
             return new MultiChannelWPEDereverberation(subbands_num, channels_num, lower_num, upper_num, iterations_num, load_db, band_width, diagonal_bias, samplerate);
           }), py::arg("subbands_num"), py::arg("channels_num"), py::arg("lower_num"), py::arg("upper_num"), py::arg("iterations_num") = 2,
           py::arg("load_db") = -20.0, py::arg("band_width") = 0.0, py::arg("diagonal_bias") = 0.0, py::arg("samplerate") = 16000.0)
      .def("size", &MultiChannelWPEDereverberation::size)
      .def("reset", &MultiChannelWPEDereverberation::reset)
      .def("set_input", [](MultiChannelWPEDereverberation& w, py::object s) { VectorComplexFeatureStreamPtr p = as_cstream(s); w.set_input(p); })
      .def("estimate_filter", &MultiChannelWPEDereverberation::estimate_filter, py::arg("start_frame_no") = 0, py::arg("frame_num") = -1)
      .def("reset_filter", &MultiChannelWPEDereverberation::reset_filter)
      .def("next_speaker", &MultiChannelWPEDereverberation::next_speaker)
      .def("print_objective_func", &MultiChannelWPEDereverberation::print_objective_func)
      .def("frame_no", &MultiChannelWPEDereverberation::frame_no);
  py::class_<MultiChannelWPEDereverberationFeature, VectorComplexFeatureStream, cref<MultiChannelWPEDereverberationFeature>>(m, "MultiChannelWPEDereverberationFeaturePtr")
      .def(py::init([](MultiChannelWPEDereverberation* source, unsigned channel_no, unsigned primary_channel_no, const std::string& nm) {
             MultiChannelWPEDereverberationPtr p(source);
             return new MultiChannelWPEDereverberationFeature(p, channel_no, primary_channel_no, nm);
           }), py::arg("source"), py::arg("channel_no"), py::arg("primary_channel_no") = 0, py::arg("nm") = "MultiChannelWPEDereverberationFeature");
  py::class_<SingleChannelWPEDereverberationFeature, VectorComplexFeatureStream, cref<SingleChannelWPEDereverberationFeature>>(m, "SingleChannelWPEDereverberationFeaturePtr")
      .def(py::init([](py::object samples, unsigned lower_num, unsigned upper_num, unsigned iterations_num, double load_db, double band_width,
                       double samplerate, const std::string& nm) {
             VectorComplexFeatureStreamPtr p = as_cstream(samples);
             return new SingleChannelWPEDereverberationFeature(p, lower_num, upper_num, iterations_num, load_db, band_width, samplerate, nm);
           }), py::arg("samples"), py::arg("lower_num"), py::arg("upper_num"), py::arg("iterations_num") = 2, py::arg("load_db") = -20.0,
           py::arg("band_width") = 0.0, py::arg("samplerate") = 16000.0, py::arg("nm") = "SingleChannelWPEDereverberationFeature")
      .def("estimate_filter", &SingleChannelWPEDereverberationFeature::estimate_filter, py::arg("start_frame_no") = 0, py::arg("frame_num") = -1)
      .def("reset_filter", &SingleChannelWPEDereverberationFeature::reset_filter)
      .def("next_speaker", &SingleChannelWPEDereverberationFeature::next_speaker)
      .def("print_objective_func", &SingleChannelWPEDereverberationFeature::print_objective_func);

  // ---- aec/aec.h (keyword names: aec/aec.i; the NLMS node calls its sources `original` and `distorted`)
  py::class_<AcousticEchoCancellationNode_, VectorComplexFeatureStream, cref<AcousticEchoCancellationNode_>>(m, "AcousticEchoCancellationNode")
      .def("set_block_frames", &AcousticEchoCancellationNode_::set_block_frames, py::arg("n"))
      .def("block_frames", &AcousticEchoCancellationNode_::block_frames)
      .def("sample_num", &AcousticEchoCancellationNode_::sample_num)
      .def("block", [](AcousticEchoCancellationNode_& n) { return block_of(n); })
      .def("filter_coefficients", [](AcousticEchoCancellationNode_& n, unsigned fbinX) {
             const std::vector<double> r = n.filter_coefficients(fbinX);
             py::array_t<std::complex<double>> a((py::ssize_t)(r.size() / 2));
             memcpy(static_cast<void*>(a.mutable_data()), r.data(), sizeof(double) * r.size());
             return a;
           }, py::arg("fbinX"))
      .def("state_covariance", [](AcousticEchoCancellationNode_& n, unsigned fbinX) {
             const std::vector<double> r = n.state_covariance(fbinX);
             const py::ssize_t P = (py::ssize_t)n.sample_num();
             py::array_t<std::complex<double>> a({P, P});
             memcpy(static_cast<void*>(a.mutable_data()), r.data(), sizeof(double) * r.size());
             return a;
           }, py::arg("fbinX"))
      .def("observation_noise_variance", &AcousticEchoCancellationNode_::observation_noise_variance, py::arg("fbinX"));
  py::class_<NLMSAcousticEchoCancellationFeature, AcousticEchoCancellationNode_, cref<NLMSAcousticEchoCancellationFeature>>(m, "NLMSAcousticEchoCancellationFeaturePtr")
      .def(py::init([](py::object original, py::object distorted, double delta, double epsilon, double threshold, const std::string& nm) {
             return new NLMSAcousticEchoCancellationFeature(as_cstream(original), as_cstream(distorted), delta, epsilon, threshold, nm);
           }), py::arg("original"), py::arg("distorted"), py::arg("delta") = 100.0, py::arg("epsilon") = 1.0E-04, py::arg("threshold") = 100.0,
           py::arg("nm") = "AEC");
  py::class_<KalmanFilterEchoCancellationFeature, AcousticEchoCancellationNode_, cref<KalmanFilterEchoCancellationFeature>>(m, "KalmanFilterEchoCancellationFeaturePtr")
      .def(py::init([](py::object played, py::object recorded, double beta, double sigma2, double threshold, const std::string& nm) {
             return new KalmanFilterEchoCancellationFeature(as_cstream(played), as_cstream(recorded), beta, sigma2, threshold, nm);
           }), py::arg("played"), py::arg("recorded"), py::arg("beta") = 0.95, py::arg("sigma2") = 100.0, py::arg("threshold") = 100.0,
           py::arg("nm") = "KFEchoCanceller");
  py::class_<BlockKalmanFilterEchoCancellationFeature, AcousticEchoCancellationNode_, cref<BlockKalmanFilterEchoCancellationFeature>>(m, "BlockKalmanFilterEchoCancellationFeaturePtr")
      .def(py::init([](py::object played, py::object recorded, unsigned sample_num, double beta, double sigmau2, double sigmak2, double threshold,
                       double amp4play, const std::string& nm) {
             return new BlockKalmanFilterEchoCancellationFeature(as_cstream(played), as_cstream(recorded), sample_num, beta, sigmau2, sigmak2, threshold,
                                                                 amp4play, nm);
           }), py::arg("played"), py::arg("recorded"), py::arg("sample_num") = 1, py::arg("beta") = 0.95, py::arg("sigmau2") = 10e-4,
           py::arg("sigmak2") = 5.0, py::arg("threshold") = 100.0, py::arg("amp4play") = 1.0, py::arg("nm") = "BlockKFEchoCanceller");
  py::class_<DTDBlockKalmanFilterEchoCancellationFeature, BlockKalmanFilterEchoCancellationFeature, cref<DTDBlockKalmanFilterEchoCancellationFeature>>(m, "DTDBlockKalmanFilterEchoCancellationFeaturePtr")
      .def(py::init([](py::object played, py::object recorded, unsigned sample_num, double beta, double sigmau2, double sigmak2, double snr_threshold,
                       double energy_threshold, double smooth, double amp4play, const std::string& nm) {
             return new DTDBlockKalmanFilterEchoCancellationFeature(as_cstream(played), as_cstream(recorded), sample_num, beta, sigmau2, sigmak2,
                                                                    snr_threshold, energy_threshold, smooth, amp4play, nm);
           }), py::arg("played"), py::arg("recorded"), py::arg("sample_num") = 1, py::arg("beta") = 0.95, py::arg("sigmau2") = 10e-4,
           py::arg("sigmak2") = 5.0, py::arg("snr_threshold") = 2.0, py::arg("energy_threshold") = 100.0, py::arg("smooth") = 0.9,
           py::arg("amp4play") = 1.0, py::arg("nm") = "DTDBlockKFEchoCanceller");

  // ---- postfilter/spectralsubtraction.h, HighPassFilter of postfilter/postfilter.h (keyword names: postfilter/postfilter.i)
  py::class_<EnhancementBlockNode_, VectorComplexFeatureStream, cref<EnhancementBlockNode_>>(m, "EnhancementBlockNode")
      .def("set_block_frames", &EnhancementBlockNode_::set_block_frames, py::arg("n"))
      .def("block_frames", &EnhancementBlockNode_::block_frames)
      .def("block_version", [](EnhancementBlockNode_& n) { return n.block_version(); })
      .def("advance_to", [](EnhancementBlockNode_& n, long frame_idx) { n.advance_to(frame_idx); }, py::arg("frame_idx"))
      .def("block", [](EnhancementBlockNode_& n) { return block_of(n); });
  py::class_<SpectralSubtractor, EnhancementBlockNode_, cref<SpectralSubtractor>>(m, "SpectralSubtractorPtr")
      .def(py::init([](unsigned fftLen, bool halfBandShift, float ft, float flooringV, const std::string& nm) {
             return new SpectralSubtractor(fftLen, halfBandShift, ft, flooringV, nm);
           }), py::arg("fftLen"), py::arg("halfBandShift") = false, py::arg("ft") = 1.0f, py::arg("flooringV") = 0.001f,
           py::arg("nm") = "SpectralSubtractor")
      .def("clear", &SpectralSubtractor::clear)
      .def("set_noise_over_estimation_factor", &SpectralSubtractor::set_noise_over_estimation_factor, py::arg("ft"))
      .def("set_channel", [](SpectralSubtractor& s, py::object chan, double alpha) { VectorComplexFeatureStreamPtr p = as_cstream(chan); s.set_channel(p, alpha); },
           py::arg("chan"), py::arg("alpha") = -1.0)
      .def("start_training", &SpectralSubtractor::start_training)
      .def("stop_training", &SpectralSubtractor::stop_training)
      .def("clear_noise_samples", &SpectralSubtractor::clear_noise_samples)
      .def("start_noise_subtraction", &SpectralSubtractor::start_noise_subtraction)
      .def("stop_noise_subtraction", &SpectralSubtractor::stop_noise_subtraction)
      .def("read_noise_file", [](SpectralSubtractor& s, const std::string& fn, unsigned idx) { return s.read_noise_file(fn, idx); }, py::arg("fn"), py::arg("idx") = 0)
      .def("write_noise_file", [](SpectralSubtractor& s, const std::string& fn, unsigned idx) { return s.write_noise_file(fn, idx); }, py::arg("fn"), py::arg("idx") = 0)
      .def("noise_psd", [](SpectralSubtractor& s, unsigned idx) {
             const std::vector<double> r = s.noise_psd(idx);
             py::array_t<double> a((py::ssize_t)r.size());
             memcpy(a.mutable_data(), r.data(), sizeof(double) * r.size());
             return a;
           }, py::arg("idx") = 0);
  py::class_<WienerFilter, EnhancementBlockNode_, cref<WienerFilter>>(m, "WienerFilterPtr")
      .def(py::init([](py::object targetSignal, py::object noiseSignal, bool halfBandShift, float alpha, float flooringV, double beta, const std::string& nm) {
             VectorComplexFeatureStreamPtr t = as_cstream(targetSignal), n = as_cstream(noiseSignal);
             return new WienerFilter(t, n, halfBandShift, alpha, flooringV, beta, nm);
           }), py::arg("targetSignal"), py::arg("noiseSignal"), py::arg("halfBandShift") = false, py::arg("alpha") = 0.0f,
           py::arg("flooringV") = 0.001f, py::arg("beta") = 1.0, py::arg("nm") = "WienerFilter")
      .def("set_noise_amplification_factor", &WienerFilter::set_noise_amplification_factor, py::arg("beta"))
      .def("start_updating_noise_PSD", &WienerFilter::start_updating_noise_PSD)
      .def("stop_updating_noise_PSD", &WienerFilter::stop_updating_noise_PSD)
      .def("target_psd", [](WienerFilter& w) {
             const std::vector<double> r = w.target_psd();
             py::array_t<double> a((py::ssize_t)r.size());
             memcpy(a.mutable_data(), r.data(), sizeof(double) * r.size());
             return a;
           })
      .def("noise_psd", [](WienerFilter& w) {
             const std::vector<double> r = w.noise_psd();
             py::array_t<double> a((py::ssize_t)r.size());
             memcpy(a.mutable_data(), r.data(), sizeof(double) * r.size());
             return a;
           });
  // (cutOffFreq = 150 is the default of the reference's Python interface, postfilter/postfilter.i:298 -- the C++ constructor has
  // none, postfilter.h:209 -- and, as there, it stands in front of a parameter without one: usable by keyword only)
  py::class_<HighPassFilter, EnhancementBlockNode_, cref<HighPassFilter>>(m, "HighPassFilterPtr")
      .def(py::init([](py::object output, float cutOffFreq, int sampleRate, const std::string& nm) {
             VectorComplexFeatureStreamPtr p = as_cstream(output);
             return new HighPassFilter(p, cutOffFreq, sampleRate, nm);
           }), py::arg("output"), py::arg("cutOffFreq") = 150.0f, py::arg("sampleRate"), py::arg("nm") = "HighPassFilter")
      .def("cutoff_bin", &HighPassFilter::cutoff_bin);

  // ---- postfilter/binauralprocessing.h (keyword names: postfilter/postfilter.i:321-558).  dPowerCoeff defaults to the header's
  // 1/15.0 (IIDThresholdEstimator: 0.5): the .i file's integer 1/15 is 0 and makes every cost constant.
  auto dvec = [](const gsl_vector* v) -> py::object {
    if (!v) return py::none();
    py::array_t<double> a((py::ssize_t)v->size);
    for (size_t i = 0; i < v->size; i++) a.mutable_data()[i] = gsl_vector_get(v, i);
    return std::move(a);
  };
  py::class_<BinaryMaskFilter, EnhancementBlockNode_, cref<BinaryMaskFilter>>(m, "BinaryMaskFilterPtr")
      .def(py::init([](unsigned chanX, py::object srcL, py::object srcR, unsigned M, float threshold, float alpha, float dEta, const std::string& nm) {
             VectorComplexFeatureStreamPtr l = as_cstream(srcL), r = as_cstream(srcR);
             return new BinaryMaskFilter(chanX, l, r, M, threshold, alpha, dEta, nm);
           }), py::arg("chanX"), py::arg("srcL"), py::arg("srcR"), py::arg("M"), py::arg("threshold"), py::arg("alpha"),
           py::arg("dEta") = 0.01f, py::arg("nm") = "BinaryMaskFilter")
      .def("set_threshold", &BinaryMaskFilter::set_threshold, py::arg("threshold"))
      .def("setThreshold", &BinaryMaskFilter::set_threshold, py::arg("threshold"))
      .def("set_thresholds", [](BinaryMaskFilter& f, const py::array_t<double, py::array::c_style | py::array::forcecast>& t) { GslVec v(t); f.set_thresholds(v.v); }, py::arg("thresholds"))
      .def("setThresholds", [](BinaryMaskFilter& f, const py::array_t<double, py::array::c_style | py::array::forcecast>& t) { GslVec v(t); f.set_thresholds(v.v); }, py::arg("thresholds"))
      .def("threshold", &BinaryMaskFilter::threshold)
      .def("getThreshold", &BinaryMaskFilter::threshold)
      .def("thresholds", [dvec](BinaryMaskFilter& f) { return dvec(f.thresholds()); })
      .def("getThresholds", [dvec](BinaryMaskFilter& f) { return dvec(f.thresholds()); })
      .def("prev_mu", [](BinaryMaskFilter& f) {
             const std::vector<float> r = f.prev_mu();
             py::array_t<float> a((py::ssize_t)r.size());
             if (!r.empty()) memcpy(a.mutable_data(), r.data(), sizeof(float) * r.size());
             return a;
           })
      .def("device_block", [](BinaryMaskFilter& f) { return block_of(f); });
  py::class_<KimBinaryMaskFilter, BinaryMaskFilter, cref<KimBinaryMaskFilter>>(m, "KimBinaryMaskFilterPtr")
      .def(py::init([](unsigned chanX, py::object srcL, py::object srcR, unsigned M, float threshold, float alpha, float dEta, float dPowerCoeff,
                       const std::string& nm) {
             VectorComplexFeatureStreamPtr l = as_cstream(srcL), r = as_cstream(srcR);
             return new KimBinaryMaskFilter(chanX, l, r, M, threshold, alpha, dEta, dPowerCoeff, nm);
           }), py::arg("chanX"), py::arg("srcL"), py::arg("srcR"), py::arg("M"), py::arg("threshold"), py::arg("alpha"),
           py::arg("dEta") = 0.01f, py::arg("dPowerCoeff") = (float)(1 / 15.0), py::arg("nm") = "KimBinaryMaskFilter");
  py::class_<IIDBinaryMaskFilter, BinaryMaskFilter, cref<IIDBinaryMaskFilter>>(m, "IIDBinaryMaskFilterPtr")
      .def(py::init([](unsigned chanX, py::object srcL, py::object srcR, unsigned M, float threshold, float alpha, float dEta, const std::string& nm) {
             VectorComplexFeatureStreamPtr l = as_cstream(srcL), r = as_cstream(srcR);
             return new IIDBinaryMaskFilter(chanX, l, r, M, threshold, alpha, dEta, nm);
           }), py::arg("chanX"), py::arg("srcL"), py::arg("srcR"), py::arg("M"), py::arg("threshold"), py::arg("alpha"),
           py::arg("dEta") = 0.01f, py::arg("nm") = "IIDBinaryMaskFilter");
  py::class_<KimITDThresholdEstimator, KimBinaryMaskFilter, cref<KimITDThresholdEstimator>>(m, "KimITDThresholdEstimatorPtr")
      .def(py::init([](py::object srcL, py::object srcR, unsigned M, float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq,
                       int sampleRate, float dEta, float dPowerCoeff, const std::string& nm) {
             VectorComplexFeatureStreamPtr l = as_cstream(srcL), r = as_cstream(srcR);
             return new KimITDThresholdEstimator(l, r, M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, nm);
           }), py::arg("srcL"), py::arg("srcR"), py::arg("M"), py::arg("minThreshold") = 0.0f, py::arg("maxThreshold") = 0.0f,
           py::arg("width") = 0.02f, py::arg("minFreq") = -1.0f, py::arg("maxFreq") = -1.0f, py::arg("sampleRate") = -1,
           py::arg("dEta") = 0.01f, py::arg("dPowerCoeff") = (float)(1 / 15.0), py::arg("nm") = "KimITDThresholdEstimator")
      .def("calc_threshold", &KimITDThresholdEstimator::calc_threshold)
      .def("calcThreshold", &KimITDThresholdEstimator::calc_threshold)
      .def("cost_function", [dvec](KimITDThresholdEstimator& e) { return dvec(e.cost_function()); })
      .def("getCostFunction", [dvec](KimITDThresholdEstimator& e) { return dvec(e.cost_function()); })
      .def("num_candidates", &KimITDThresholdEstimator::num_candidates)
      .def("candidates", [](KimITDThresholdEstimator& e) {
             const std::vector<float>& c = e.candidates();
             py::array_t<float> a((py::ssize_t)c.size());
             if (!c.empty()) memcpy(a.mutable_data(), c.data(), sizeof(float) * c.size());
             return a;
           })
      .def("min_fbin", &KimITDThresholdEstimator::min_fbin)
      .def("max_fbin", &KimITDThresholdEstimator::max_fbin)
      .def("num_samples", &KimITDThresholdEstimator::num_samples);
  py::class_<IIDThresholdEstimator, KimITDThresholdEstimator, cref<IIDThresholdEstimator>>(m, "IIDThresholdEstimatorPtr")
      .def(py::init([](py::object srcL, py::object srcR, unsigned M, float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq,
                       int sampleRate, float dEta, float dPowerCoeff, const std::string& nm) {
             VectorComplexFeatureStreamPtr l = as_cstream(srcL), r = as_cstream(srcR);
             return new IIDThresholdEstimator(l, r, M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, nm);
           }), py::arg("srcL"), py::arg("srcR"), py::arg("M"), py::arg("minThreshold") = 0.0f, py::arg("maxThreshold") = 0.0f,
           py::arg("width") = 0.02f, py::arg("minFreq") = -1.0f, py::arg("maxFreq") = -1.0f, py::arg("sampleRate") = -1,
           py::arg("dEta") = 0.01f, py::arg("dPowerCoeff") = 0.5f, py::arg("nm") = "IIDThresholdEstimator");
  py::class_<FDIIDThresholdEstimator, BinaryMaskFilter, cref<FDIIDThresholdEstimator>>(m, "FDIIDThresholdEstimatorPtr")
      .def(py::init([](py::object src_left, py::object src_right, unsigned M, float min_threshold, float max_threshold, float width, float deta,
                       float dpowercoeff, const std::string& nm) {
             VectorComplexFeatureStreamPtr l = as_cstream(src_left), r = as_cstream(src_right);
             return new FDIIDThresholdEstimator(l, r, M, min_threshold, max_threshold, width, deta, dpowercoeff, nm);
           }), py::arg("src_left"), py::arg("src_right"), py::arg("M"), py::arg("min_threshold") = 0.0f, py::arg("max_threshold") = 0.0f,
           py::arg("width") = 1000.0f, py::arg("deta") = 0.01f, py::arg("dpowercoeff") = (float)(1 / 15.0),
           py::arg("nm") = "FDIIDThresholdEstimator")
      .def("calc_threshold", &FDIIDThresholdEstimator::calc_threshold)
      .def("calcThreshold", &FDIIDThresholdEstimator::calc_threshold)
      .def("cost_function", [dvec](FDIIDThresholdEstimator& e, unsigned freqX) { return dvec(e.cost_function(freqX)); }, py::arg("freqX"))
      .def("getCostFunction", [dvec](FDIIDThresholdEstimator& e, unsigned freqX) { return dvec(e.cost_function(freqX)); }, py::arg("freqX"))
      .def("num_candidates", &FDIIDThresholdEstimator::num_candidates)
      .def("candidates", [](FDIIDThresholdEstimator& e) {
             const std::vector<float>& c = e.candidates();
             py::array_t<float> a((py::ssize_t)c.size());
             if (!c.empty()) memcpy(a.mutable_data(), c.data(), sizeof(float) * c.size());
             return a;
           });

  // ---- sad/sad.h (sad/sad.i): the energy family of the voice activity detection.  A metric is any bound VADMetric.
  auto as_metric = [](const py::object& o) {
    if (!py::isinstance<VADMetric>(o)) throw jparameter_error("expected a VAD metric (VADMetricPtr)");
    return VADMetricPtr(o.cast<VADMetric*>());
  };
  py::class_<VADMetric, cref<VADMetric>>(m, "VADMetricPtr")
      .def("next", [](VADMetric& v, int frame_no) { return v.next(frame_no); }, py::arg("frame_no") = -5)
      .def("__next__", [](VADMetric& v) { return v.next(-5); })
      .def("__iter__", [](py::object self) { self.attr("reset")(); return self; })
      .def("reset", [](VADMetric& v) { v.reset(); })
      .def("score", [](VADMetric& v) { return v.score(); })
      .def("next_speaker", [](VADMetric& v) { v.next_speaker(); })
      .def("nextSpeaker", [](VADMetric& v) { v.next_speaker(); })
      .def("frame_no", [](VADMetric& v) { return v.frame_no(); })
      .def("set_block_frames", [](VADMetric& v, long n) { v.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](VADMetric& v) { return v.block_frames(); })
      .def("launches", [](VADMetric& v) { return v.launches(); });
  py::class_<EnergyVADMetric, VADMetric, cref<EnergyVADMetric>>(m, "EnergyVADMetricPtr")
      .def(py::init([](py::object source, double initialEnergy, double threshold, unsigned headN, unsigned tailN, unsigned energiesN,
                       const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(source);
             return new EnergyVADMetric(sp, initialEnergy, threshold, headN, tailN, energiesN, nm);
           }), py::arg("source"), py::arg("initialEnergy") = 5.0e+07, py::arg("threshold") = 0.5, py::arg("headN") = 4, py::arg("tailN") = 10,
           py::arg("energiesN") = 200, py::arg("nm") = "Energy VAD Metric")
      .def("energy_percentile", &EnergyVADMetric::energy_percentile, py::arg("percentile") = 50.0)
      .def("energyPercentile", &EnergyVADMetric::energy_percentile, py::arg("percentile") = 50.0);
  py::class_<PowerSpectrumVADMetric, VADMetric, cref<PowerSpectrumVADMetric>>(m, "PowerSpectrumVADMetricPtr")
      .def(py::init([](unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const std::string& nm) {
             return new PowerSpectrumVADMetric(fftLen, sampleRate, lowCutoff, highCutoff, nm);
           }), py::arg("fftLen"), py::arg("sampleRate") = 16000.0, py::arg("lowCutoff") = -1.0, py::arg("highCutoff") = -1.0,
           py::arg("nm") = "Power Spectrum VAD Metric")
      .def("set_channel", [](PowerSpectrumVADMetric& v, py::object chan) { v.set_channel(as_fstream(chan)); }, py::arg("chan"))
      .def("setChannel", [](PowerSpectrumVADMetric& v, py::object chan) { v.set_channel(as_fstream(chan)); }, py::arg("chan"))
      .def("clear_channel", &PowerSpectrumVADMetric::clear_channel)
      .def("clearChannel", &PowerSpectrumVADMetric::clear_channel)
      .def("set_E0", &PowerSpectrumVADMetric::set_E0, py::arg("E0"))
      .def("setE0", &PowerSpectrumVADMetric::set_E0, py::arg("E0"))
      .def("get_metrics", [](PowerSpectrumVADMetric& v) -> py::object {
             const gsl_vector* p = v.get_metrics();
             if (!p) return py::none();
             return py::array_t<double>((py::ssize_t)p->size, p->data);
           })
      .def("getMetrics", [](PowerSpectrumVADMetric& v) -> py::object {
             const gsl_vector* p = v.get_metrics();
             if (!p) return py::none();
             return py::array_t<double>((py::ssize_t)p->size, p->data);
           })
      .def("lowX", &PowerSpectrumVADMetric::lowX)
      .def("highX", &PowerSpectrumVADMetric::highX)
      .def("binN", &PowerSpectrumVADMetric::binN);
  py::class_<NormalizedEnergyMetric, PowerSpectrumVADMetric, cref<NormalizedEnergyMetric>>(m, "NormalizedEnergyMetricPtr")
      .def(py::init([](unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const std::string& nm) {
             return new NormalizedEnergyMetric(fftLen, sampleRate, lowCutoff, highCutoff, nm);
           }), py::arg("fftLen"), py::arg("sampleRate") = 16000.0, py::arg("lowCutoff") = -1.0, py::arg("highCutoff") = -1.0,
           py::arg("nm") = "NormalizedEnergyMetric");
  py::class_<TSPSVADMetric, PowerSpectrumVADMetric, cref<TSPSVADMetric>>(m, "TSPSVADMetricPtr")
      .def(py::init([](unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const std::string& nm) {
             return new TSPSVADMetric(fftLen, sampleRate, lowCutoff, highCutoff, nm);
           }), py::arg("fftLen"), py::arg("sampleRate") = 16000.0, py::arg("lowCutoff") = -1.0, py::arg("highCutoff") = -1.0,
           py::arg("nm") = "TSPS VAD Metric");
  py::class_<VAD, cref<VAD>>(m, "VADPtr")
      .def("next", [](VAD& v, int frame_no) { return v.next(frame_no); }, py::arg("frame_no") = -5)
      .def("__next__", [](VAD& v) { return v.next(-5); })
      .def("__iter__", [](py::object self) { self.attr("reset")(); return self; })
      .def("reset", [](VAD& v) { v.reset(); })
      .def("frame", [](py::object self) { return view(self.cast<VAD&>().frame(), self); })
      .def("next_speaker", [](VAD& v) { v.next_speaker(); })
      .def("nextSpeaker", [](VAD& v) { v.next_speaker(); })
      .def("frame_no", [](VAD& v) { return v.frame_no(); });
  py::class_<SimpleEnergyVAD, VAD, cref<SimpleEnergyVAD>>(m, "SimpleEnergyVADPtr")
      .def(py::init([](py::object samp, double threshold, double gamma) {
             VectorComplexFeatureStreamPtr sp = as_cstream(samp);
             return new SimpleEnergyVAD(sp, threshold, gamma);
           }), py::arg("samp"), py::arg("threshold"), py::arg("gamma") = 0.98)
      .def("spectral_energy", &SimpleEnergyVAD::spectral_energy)
      .def("set_block_frames", [](SimpleEnergyVAD& v, long n) { v.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](SimpleEnergyVAD& v) { return v.block_frames(); })
      .def("launches", [](SimpleEnergyVAD& v) { return v.launches(); });
  py::class_<HangoverVADFeature, VectorFloatFeatureStream, cref<HangoverVADFeature>>(m, "HangoverVADFeaturePtr")
      .def(py::init([as_metric](py::object source, py::object metric, double threshold, unsigned headN, unsigned tailN, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(source);
             return new HangoverVADFeature(sp, as_metric(metric), threshold, headN, tailN, nm);
           }), py::arg("source"), py::arg("metric"), py::arg("threshold") = 0.5, py::arg("headN") = 4, py::arg("tailN") = 10,
           py::arg("nm") = "Hangover VAD Feature")
      .def("reset", [](HangoverVADFeature& f) { f.reset(); })
      .def("next_speaker", [](HangoverVADFeature& f) { f.next_speaker(); })
      .def("nextSpeaker", [](HangoverVADFeature& f) { f.next_speaker(); })
      .def("prefixN", &HangoverVADFeature::prefixN)
      .def("set_block_frames", [](HangoverVADFeature& f, long n) { f.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](HangoverVADFeature& f) { return f.block_frames(); })
      .def("launches", [](HangoverVADFeature& f) { return f.launches(); });
  py::class_<HangoverMIVADFeature, HangoverVADFeature, cref<HangoverMIVADFeature>>(m, "HangoverMIVADFeaturePtr")
      .def(py::init([as_metric](py::object source, py::object energyMetric, py::object mutualInformationMetric, py::object powerMetric,
                                double energyThreshold, double mutualInformationThreshold, double powerThreshold, unsigned headN,
                                unsigned tailN, const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(source);
             return new HangoverMIVADFeature(sp, as_metric(energyMetric), as_metric(mutualInformationMetric), as_metric(powerMetric),
                                             energyThreshold, mutualInformationThreshold, powerThreshold, headN, tailN, nm);
           }), py::arg("source"), py::arg("energyMetric"), py::arg("mutualInformationMetric"), py::arg("powerMetric"),
           py::arg("energyThreshold") = 0.5, py::arg("mutualInformationThreshold") = 0.5, py::arg("powerThreshold") = 0.5,
           py::arg("headN") = 4, py::arg("tailN") = 10, py::arg("nm") = "Hangover MIVAD Feature")
      .def("decision_metric", &HangoverMIVADFeature::decision_metric)
      .def("decisionMetric", &HangoverMIVADFeature::decision_metric);
  py::class_<HangoverMultiStageVADFeature, HangoverVADFeature, cref<HangoverMultiStageVADFeature>>(m, "HangoverMultiStageVADFeaturePtr")
      .def(py::init([as_metric](py::object source, py::object energyMetric, double energyThreshold, unsigned headN, unsigned tailN,
                                const std::string& nm) {
             VectorFloatFeatureStreamPtr sp = as_fstream(source);
             return new HangoverMultiStageVADFeature(sp, as_metric(energyMetric), energyThreshold, headN, tailN, nm);
           }), py::arg("source"), py::arg("energyMetric"), py::arg("energyThreshold") = 0.5, py::arg("headN") = 4, py::arg("tailN") = 10,
           py::arg("nm") = "HangoverMultiStageVADFeature")
      .def("decision_metric", &HangoverMultiStageVADFeature::decision_metric)
      .def("decisionMetric", &HangoverMultiStageVADFeature::decision_metric)
      .def("set_metric", [as_metric](HangoverMultiStageVADFeature& f, py::object metricPtr, double threshold) { f.set_metric(as_metric(metricPtr), threshold); },
           py::arg("metricPtr"), py::arg("threshold"))
      .def("setMetric", [as_metric](HangoverMultiStageVADFeature& f, py::object metricPtr, double threshold) { f.set_metric(as_metric(metricPtr), threshold); },
           py::arg("metricPtr"), py::arg("threshold"));

  // ---- objective_measure/objective_measure.h (objective_measure/objective_measure.i)
  py::class_<SNR, cref<SNR>>(m, "SNRPtr")
      .def(py::init([]() { return new SNR(); }))
      .def("getSNR", &SNR::getSNR, py::arg("fn1"), py::arg("fn2"), py::arg("normalizationOption"), py::arg("chX") = 1,
           py::arg("samplerate") = 16000, py::arg("cfrom") = -1, py::arg("to") = -1)
      .def("getSNR2", [](SNR& s, py::array_t<float, py::array::c_style | py::array::forcecast> original,
                         py::array_t<float, py::array::c_style | py::array::forcecast> enhanced, int normalizationOption) {
             gsl_vector_float a, b;
             a.size = (size_t)original.size(); a.stride = 1; a.data = const_cast<float*>(original.data());
             b.size = (size_t)enhanced.size(); b.stride = 1; b.data = const_cast<float*>(enhanced.data());
             return s.getSNR2(&a, &b, normalizationOption);
           }, py::arg("original"), py::arg("enhanced"), py::arg("normalizationOption"))
      .def("stats", [](SNR& s) {
             py::array_t<double> a(6);
             std::copy(s.stats(), s.stats() + 6, a.mutable_data());
             return a;
           });
  py::class_<ItakuraSaitoMeasurePS, cref<ItakuraSaitoMeasurePS>>(m, "ItakuraSaitoMeasurePSPtr")
      .def(py::init([](unsigned fftLen, unsigned r, unsigned windowType, const std::string& nm) {
             return new ItakuraSaitoMeasurePS(fftLen, r, windowType, nm);
           }), py::arg("fftLen"), py::arg("r") = 1, py::arg("windowType") = 1, py::arg("nm") = "ItakuraSaitoMeasurePS")
      .def("getDistance", &ItakuraSaitoMeasurePS::getDistance, py::arg("fn1"), py::arg("fn2"), py::arg("chX") = 1,
           py::arg("samplerate") = 16000, py::arg("bframe") = 0, py::arg("eframe") = -1)
      .def("frameShiftLength", &ItakuraSaitoMeasurePS::frameShiftLength)
      .def("frames", &ItakuraSaitoMeasurePS::frames)
      .def("distance", &ItakuraSaitoMeasurePS::distance);

  // ---- localization/localization.h (localization/localization.i:128-260)
  auto as_sgb = [](py::object o) { return SearchGridBuilderPtr(o.cast<SearchGridBuilder*>()); };
  py::class_<SearchGridBuilder, cref<SearchGridBuilder>>(m, "SearchGridBuilderPtr")
      .def(py::init([](int nChan, bool isFarField, unsigned int samplingFreq) { return new SearchGridBuilder(nChan, isFarField, samplingFreq); }),
           py::arg("nChan"), py::arg("isFarField"), py::arg("samplingFreq") = 16000u)
      .def("nextSearchGrid", [](SearchGridBuilder& g) { return g.nextSearchGrid(); })
      .def("getTimeDelays", [](py::object self) -> py::object {
             const gsl_vector* v = self.cast<SearchGridBuilder&>().getTimeDelays();
             if (!v) return py::none();
             return view(v, self); })
      .def("getSearchPosition", [](py::object self) { return view(self.cast<SearchGridBuilder&>().getSearchPosition(), self); })
      .def("maxTimeDelay", [](SearchGridBuilder& g) { return g.maxTimeDelay(); })
      .def("chanN", [](SearchGridBuilder& g) { return g.chanN(); })
      .def("samplingFrequency", [](SearchGridBuilder& g) { return g.samplingFrequency(); })
      .def("reset", [](SearchGridBuilder& g) { g.reset(); });
  py::class_<SGB4LinearArray, SearchGridBuilder, cref<SGB4LinearArray>>(m, "SGB4LinearArrayPtr")
      .def(py::init([](int nChan, bool isFarField, unsigned int samplingFreq) { return new SGB4LinearArray(nChan, isFarField, samplingFreq); }),
           py::arg("nChan"), py::arg("isFarField"), py::arg("samplingFreq") = 16000u)
      .def("setDistanceBtwMicrophones", [](SGB4LinearArray& g, float distance) { g.setDistanceBtwMicrophones(distance); }, py::arg("distance"))
      .def("setPositionsOfMicrophones", [](SGB4LinearArray& g, py::array_t<double, py::array::c_style | py::array::forcecast> mpos) {
             GslMat mp(mpos);
             g.setPositionsOfMicrophones(mp.m);
           }, py::arg("mpos"));
  py::class_<MCCLocalizer, VectorFeatureStream, cref<MCCLocalizer>>(m, "MCCLocalizerPtr")
      .def(py::init([as_sgb](py::object sgbPtr, size_t maxSource, const std::string& nm) {
             SearchGridBuilderPtr g = as_sgb(sgbPtr);
             return new MCCLocalizer(g, maxSource, nm);
           }), py::arg("sgbPtr"), py::arg("maxSource") = 1, py::arg("nm") = "MCCSourceLocalizer")
      .def("reset", [](MCCLocalizer& l) { l.reset(); })
      .def("setChannel", [](MCCLocalizer& l, py::object chan) { VectorFloatFeatureStreamPtr c = as_fstream(chan); l.setChannel(c); }, py::arg("chan"))
      .def("getDelayedSample", [](MCCLocalizer& l, int chanX) { return l.getDelayedSample(chanX); }, py::arg("chanX"))
      .def("getMaxMCCC", [](MCCLocalizer& l) { return l.getMaxMCCC(); })
      .def("getPosition", [](py::object self) { return view(self.cast<MCCLocalizer&>().getPosition(), self); })
      .def("getNthBestDelayedSample", [](MCCLocalizer& l, int nth, int chanX) { return l.getNthBestDelayedSample(nth, chanX); }, py::arg("nth"), py::arg("chanX"))
      .def("getNthBestMCCC", [](MCCLocalizer& l, int nth) { return l.getNthBestMCCC(nth); }, py::arg("nth"))
      .def("getNthBestPosition", [](py::object self, int nth) { return view(self.cast<MCCLocalizer&>().getNthBestPosition(nth), self); }, py::arg("nth"))
      .def("getEigenValues", [](py::object self) { return view(self.cast<MCCLocalizer&>().getEigenValues(), self); })
      .def("getR", [](MCCLocalizer& l) { return dense_of(l.getR()); })
      .def("set_block_frames", [](MCCLocalizer& l, long n) { l.set_block_frames(n); }, py::arg("n"))
      .def("block_frames", [](MCCLocalizer& l) { return l.block_frames(); })
      .def("launches", [](MCCLocalizer& l) { return l.launches(); });
  py::class_<MCCCalculator, MCCLocalizer, cref<MCCCalculator>>(m, "MCCCalculatorPtr")
      .def(py::init([as_sgb](py::object sgbPtr, bool normalizeVariance, const std::string& nm) {
             SearchGridBuilderPtr g = as_sgb(sgbPtr);
             return new MCCCalculator(g, normalizeVariance, nm);
           }), py::arg("sgbPtr"), py::arg("normalizeVariance") = true, py::arg("nm") = "MCCCalculator")
      .def("reset", [](MCCCalculator& l) { l.reset(); })
      .def("setTimeDelays", [](MCCCalculator& l, py::array_t<double, py::array::c_style | py::array::forcecast> delays) {
             GslVec d(delays);
             l.setTimeDelays(d.v);
           }, py::arg("delays"))
      .def("getMCCC", [](MCCCalculator& l) { return l.getMCCC(); })
      .def("getCostV", [](MCCCalculator& l) { return l.getCostV(); })
      .def("normalizeVariance", [](MCCCalculator& l) { return l.normalizeVariance(); })
      .def("setNormalizeVariance", [](MCCCalculator& l, bool v) { l.setNormalizeVariance(v); }, py::arg("normalizeVariance"));
}
