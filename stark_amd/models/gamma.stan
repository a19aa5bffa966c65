// Gamma regression with the log link: a positive, right-skewed response with mean exp(alpha + x * beta) and
// variance mean^2 / shape (claim sizes, costs, durations).  Flat priors.
data {
  int<lower=0> N;
  int<lower=0> K;
  matrix[N, K] x;
  vector<lower=0>[N] y;
}
parameters {
  real alpha;
  vector[K] beta;
  real<lower=0> shape;
}
model {
  y ~ gamma(shape, shape ./ exp(alpha + x * beta));
}
